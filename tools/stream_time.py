"""What a streamed request costs: time to the first packet and total time, for a streaming session (infer.open_stream) with
lookahead 0 and 1 against the sequential `infer_batch_process(streaming=True)` loop, in one process.

    python tools/stream_time.py [--runs 30] [--nfe 16] [--precision f16p] [--granule 64] [--out-rate 24000] [--format f32] [--out FILE.json]

F5-TTS Base with synthetic weights, Vocos 24 kHz, length buckets on (graphs prepared ahead by the session's warm_up), a 10 s
prompt of 24 kHz mono noise with a 100-byte text (10 bytes per second: max_chars 150, few 75, min 37) and a request of 16
sentences of 36 bytes, which a first package cuts into 6 chunks (1, 1, 2, 4, 4 and 4 sentences).  Every leg speaks the same chunks:
  sequential   the reference's loop: per chunk the prompt prepared on the host, its mel, an eager sample(), the vocoder, the
               waveform to the host, then sliced into packets of 2048
  lookahead 0  the session: the prompt from the bank, per chunk sample(), ragged decode, join, deliver, one async copy; the host
               waits for a chunk's copy before it enqueues the next chunk
  lookahead 1  the same with the next chunk enqueued before the wait
The legs alternate inside every round; a round is timed with a host clock from the call to the arrival of a packet on the host
(the packet's bytes are there: the generators hand out host arrays).  Reports the median over --runs rounds after two warm-up
rounds, the spread (min, max), and whether the session's f32 24 kHz packets equal the sequential loop's bit for bit."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import f5_tts_amd as P  # noqa: E402
from f5_tts_amd import infer as I  # noqa: E402

DEV = "cuda:0"
REF_TEXT = ("This prompt has exactly one hundred bytes of text. " * 2)[:99] + "."
TEXT = " ".join("Sentence number %02d has thirtysix b." % i for i in range(16))


def timed(gen):
    """(ms to the first packet, ms to the end, packets)."""
    t0 = time.perf_counter()
    first, packets = None, []
    for packet, _rate in gen:
        if first is None:
            first = (time.perf_counter() - t0) * 1e3
        packets.append(packet)
    return first, (time.perf_counter() - t0) * 1e3, packets


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--nfe", type=int, default=16)
    ap.add_argument("--precision", default="f16p")
    ap.add_argument("--granule", type=int, default=64)
    ap.add_argument("--out-rate", type=int, default=24000)
    ap.add_argument("--format", default="f32")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("stream_time.py measures on the GPU: none is visible")

    tr = P.DiT(**P.config.F5TTS_BASE, text_num_embeds=P.config.VOCAB_SIZE + 1, mel_dim=100, precision=args.precision).init_synthetic(seed=0)
    model = P.CFM(transformer=tr, mel_spec_module=P.mel.MelSpec()).to(DEV)
    voc = P.Vocos(P.config.VOCOS_24K).init_synthetic(seed=1).to(DEV)
    tr.set_length_buckets(args.granule)
    audio = torch.randn(1, 240000, generator=torch.Generator().manual_seed(5)) * 0.05
    kw = dict(nfe_step=args.nfe, cfg_strength=2.0, sway_sampling_coef=-1.0, seed=0)
    bank = I.prepare_voices(model, {"main": dict(ref_audio=(audio, 24000), ref_text=REF_TEXT)})
    chunks = I.stream_chunks(TEXT, REF_TEXT, 10.0, True)
    assert len(REF_TEXT.encode()) == 100 and [c.count(".") for c in chunks] == [1, 1, 2, 4, 4, 4], chunks

    sessions = {k: I.open_stream(model, voc, (bank, "main"), out_rate=args.out_rate, sample_format=args.format, lookahead=k, **kw)
                for k in (0, 1)}
    t0 = time.perf_counter()
    sessions[0].warm_up()
    torch.cuda.synchronize()
    warm_ms = (time.perf_counter() - t0) * 1e3

    def sequential():
        return I.infer_batch_process((audio, 24000), REF_TEXT, chunks, model, voc, streaming=True, chunk_size=2048, **kw)

    def session(k):
        sessions[k].reset()
        return sessions[k].stream(TEXT)

    legs = {"sequential": sequential, "lookahead_0": lambda: session(0), "lookahead_1": lambda: session(1)}
    times = {name: [] for name in legs}
    kept = {}
    tr.graph_stats(reset=True)
    for r in range(args.runs + 2):
        for name, make in legs.items():
            first, total, packets = timed(make())
            torch.cuda.synchronize()
            if r >= 2:
                times[name].append((first, total))
            kept[name] = packets
    stats = tr.graph_stats()

    audio_s = sum(len(p) for p in kept["sequential"]) / 24000
    rec = {"tool": "stream_time", "precision": args.precision, "nfe": args.nfe, "granule": args.granule, "runs": args.runs,
           "out_rate": args.out_rate, "format": args.format, "chunks": len(chunks), "chunk_bytes": [len(c.encode()) for c in chunks],
           "audio_seconds": round(audio_s, 2), "warm_up_ms": round(warm_ms, 1), "graph_stats": stats}
    for name, ts in times.items():
        f, t = [x[0] for x in ts], [x[1] for x in ts]
        rec[name] = {"first_packet_ms_median": round(statistics.median(f), 2), "first_packet_ms_min_max": [round(min(f), 2), round(max(f), 2)],
                     "total_ms_median": round(statistics.median(t), 2), "total_ms_min_max": [round(min(t), 2), round(max(t), 2)],
                     "packets": len(kept[name])}
    if args.out_rate == 24000 and args.format == "f32":
        a, b = np.concatenate(kept["sequential"]), np.concatenate(kept["lookahead_1"])
        rec["session_equals_sequential_bits"] = bool(a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32)))
        rec["session_vs_sequential_linf"] = float(np.abs(a - b).max()) if a.shape == b.shape else None
    a, b = np.concatenate(kept["lookahead_0"]), np.concatenate(kept["lookahead_1"])
    rec["lookahead_results_equal"] = bool(np.array_equal(a, b))
    for name in times:
        print(f"{name:12s} first packet {rec[name]['first_packet_ms_median']:9.2f} ms   total {rec[name]['total_ms_median']:9.2f} ms")
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
