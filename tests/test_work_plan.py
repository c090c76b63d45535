"""CPU: the engine's work-buffer plan (f5k_work_plan runs the real carve_into and second_half on a dry-run arena) against an
independent statement of how many bytes one backbone forward writes into each buffer, from the kernels' strides and element types:

    T (xn, q, k, ao, vt, ffh, and acat / cat2 unless said otherwise) is 4 bytes for f32 and f16x3, 2 bytes for bf16, f16 and f16p
    f16p packs the input rows (acat) and the long-skip concat (cat2) as f32, and writes its final-norm rows as f32 (into c1, or the
    UNetT's first skip slot)
    f8 (DiT only) is f16p plus the block GEMM's e4m3 A operand: a8, one code byte per element at rows of max(D, F, inner), and a8s,
    one scale byte per row
    h, c1, x, pred, skips, pred_all are f32; the UNetT input embedding, f32, is written into cat2 before the first concat
    v^T rows are Npad = round_up(tokens of the RESERVATION, 64) apart

Invariants, for every precision x backbone x reservation x call shape inside it:
 1. what a forward of the call's 2 B batch rows writes lies inside the buffer's own region (its offset .. the next buffer's offset);
 2. DiT under split CFG (F5_SPLIT_CFG=1: the two halves as two concurrent stream chains of B batch rows each): the side chain's
    extent lies inside the same region and is disjoint from the main chain's;
 3. the UNetT's f32 input embedding fits the cat2 it aliases."""
import pytest

from f5_tts_amd import _lib
from gpu_util import k_work_plan

PRECS = ("f32", "f16x3", "bf16", "f16", "f16p", "f8")   # (f8: the two DiT archs; f5_create refuses it for the UNetT)
ARCHS = {"dit": (_lib.F5_BACKBONE_DIT, 0),
         "dit_qknorm_longskip": (_lib.F5_BACKBONE_DIT, _lib.F5_OPT_QK_RMSNORM | _lib.F5_OPT_LONG_SKIP),
         "unett": (_lib.F5_BACKBONE_UNETT, 0)}
DIM, DEPTH, HEADS, FF, DT, MEL = 256, 4, 6, 512, 64, 100   # heads * 64 != dim: q / k / ao strides differ from the stream's
STEPS = 4


def config(prec, arch):
    c = _lib.f5_config()
    c.backbone, c.options = ARCHS[arch]
    c.precision = _lib.PRECISIONS[prec]
    c.dim, c.depth, c.heads, c.dim_head, c.ff_dim, c.text_dim, c.mel_dim = DIM, DEPTH, HEADS, 64, FF, DT, MEL
    c.conv_layers, c.pe_attn_head, c.text_num_embeds, c.max_pos = 0, -1, 40, 4096
    return c


def round_up(v, a):
    return (v + a - 1) // a * a


def written_bytes(prec, arch, res_N, Bp, N):
    """{buffer: bytes one forward over Bp batch rows of N frames writes, from the buffer's start}."""
    unett = arch == "unett"
    sT = 4 if prec in ("f32", "f16x3") else 2
    io = 4 if prec in ("f16p", "f8") else sT  # the element size of acat and of the long-skip cat2
    kin_pad = round_up(2 * MEL + DT, 64)
    inner = HEADS * 64
    tok, res_tok = (N + 1, res_N + 1) if unett else (N, res_N)   # the UNetT prepends the time token
    rows_in, rows = Bp * N, Bp * tok
    npad = round_up(res_tok, 64)
    w = {"acat": rows_in * kin_pad * io,
         "h": rows_in * DIM * 4, "c1": rows_in * DIM * 4,        # (f16p DiT: c1 then holds the final norm's f32 rows, the same bytes)
         "x": rows * DIM * 4, "pred": rows_in * MEL * 4,
         "xn": rows * DIM * sT, "q": rows * inner * sT, "k": rows * inner * sT, "ao": rows * inner * sT,
         "vt": Bp * HEADS * 64 * npad * sT, "ffh": rows * FF * sT}
    if prec == "f8":   # the block GEMM's e4m3 A operand: codes at the pitch of the widest K, one scale byte per row
        w["a8"] = rows * max(DIM, FF, inner)
        w["a8s"] = rows
    if arch == "dit_qknorm_longskip":
        w["cat2"] = rows * 2 * DIM * io
    if unett:
        w["cat2"] = max(rows * 2 * DIM * sT, rows_in * DIM * 4)  # the concat rows of T; before them the f32 input embedding
        w["skips"] = rows * DIM * 4 * (DEPTH // 2)
        w["pred_all"] = rows * MEL * 4
    return w


def regions(total, offs):
    """{buffer: (offset, end)}: a buffer's region runs to the next buffer's offset, the last one's to the arena's end."""
    order = sorted((o, n) for n, o in offs.items() if o is not None)
    ends = [o for o, _ in order[1:]] + [total]
    return {n: (o, e) for (o, n), e in zip(order, ends)}


def call_shapes(B, N):
    return sorted({(B, N), (1, N), (B, max(1, N // 2)), (1, 1)})


@pytest.mark.parametrize("arch", list(ARCHS))
@pytest.mark.parametrize("prec", PRECS)
def test_written_extents_fit_their_regions_and_split_halves_are_disjoint(prec, arch):
    if prec == "f8" and arch == "unett":
        with pytest.raises(_lib.F5Error, match="F5_PREC_F8 is built for the DiT backbone"):
            k_work_plan(config(prec, arch), 1, 5, STEPS, 1, 5)
        return
    bad = {}   # buffer -> findings
    note = lambda name, msg: bad.setdefault(name, []).append(msg)   # noqa: E731
    for B in (1, 3):
        for N in (5, 64, 130):
            for cb, cn in call_shapes(B, N):
                total, main, side = k_work_plan(config(prec, arch), B, N, STEPS, cb, cn)
                reg = regions(total, main)
                assert all(0 <= o < e <= total for o, e in reg.values())
                where = f"{prec} {arch} reserve {B}x{N} call {cb}x{cn}"
                # 1. one forward over both halves
                for name, nbytes in written_bytes(prec, arch, N, 2 * cb, cn).items():
                    assert main[name] is not None, f"{where}: {name} is not carved"
                    if main[name] + nbytes > reg[name][1]:
                        note(name, f"{where}: {name} writes {nbytes} bytes into a region of {reg[name][1] - main[name]}")
                # 2. split CFG: two chains of cb batch rows each
                if arch != "unett":
                    for name, nbytes in written_bytes(prec, arch, N, cb, cn).items():
                        lo, hi = reg[name]
                        m0, s0 = main[name], side[name]
                        if not (lo <= s0 and s0 + nbytes <= hi and m0 + nbytes <= hi):
                            note(name, f"{where}: split-CFG {name} leaves its region (main {m0}, side {s0}, {nbytes} bytes, region {lo}..{hi})")
                        if not (m0 + nbytes <= s0 or s0 + nbytes <= m0):
                            note(name, f"{where}: split-CFG {name} halves overlap (main {m0}, side {s0}, {nbytes} bytes each)")
                # 3. the UNetT's f32 embedding inside cat2
                else:
                    emb = 2 * cb * cn * DIM * 4
                    if main["cat2"] + emb > reg["cat2"][1]:
                        note("cat2", f"{where}: the f32 input embedding ({emb} bytes) does not fit cat2")
    assert not bad, f"buffers {sorted(bad)}: " + "; ".join(f"{v[0]} (+{len(v) - 1} more)" for v in bad.values())


def test_buffer_names_follow_the_header():
    import os
    import re

    from conftest import ROOT
    src = open(os.path.join(ROOT, "include", "f5_hip.h")).read()
    block = src[src.index("#define F5K_WORK_NAMES"):src.index("int f5k_work_plan(")]
    names = " ".join(re.findall(r'"([^"]*)"', block)).split()
    assert names == list(_lib.F5K_WORK_NAMES) and int(re.search(r"#define F5K_WORK_BUFFERS (\d+)", src).group(1)) == len(names)


def test_plan_is_the_reservation_and_refuses_calls_outside_it():
    c = config("f16p", "dit")
    total, main, side = k_work_plan(c, 3, 64, STEPS, 3, 64)
    assert list(main) == list(_lib.F5K_WORK_NAMES) and main["tdev"] == 0 and main["skips"] is None and main["cat2"] is None
    assert all(o % 256 == 0 for o in main.values() if o is not None) and total % 256 == 0
    assert k_work_plan(c, 3, 64, STEPS, 1, 5)[:2] == (total, main), "the carve follows the reservation, not the call"
    shared = [n for n in main if main[n] is not None and side[n] == main[n]]
    assert not {"acat", "h", "c1", "x", "pred", "xn", "q", "k", "ao", "vt", "ffh"} & set(shared)
    for args in ((4, 64), (3, 65), (0, 64), (3, 0)):
        with pytest.raises(_lib.F5Error):
            k_work_plan(c, 3, 64, STEPS, *args)
