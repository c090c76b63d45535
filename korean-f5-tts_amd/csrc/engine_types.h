// Engine state shared by the translation units of libf5hip.so: containers, packed weights, the f5_engine handle, the
// per-call workspace and the per-precision entry points (EngineOps<T>, instantiated once per operand type in
// engine_bf16.hip / engine_f16.hip / engine_f32.hip so that the precisions compile in parallel; F5_PREC_F16X3 is the float
// instantiation with f5_engine::split16 set).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <algorithm>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "internal.h"
#include "adapter.h"
#include "attn2.h"
#include "convpos.h"
#include "elementwise.h"
#include "flow.h"
#include "gemm_dispatch.h"
#include "mmdit.h"

using namespace f5;
#define fail f5_fail
// ------------------------------------------------------------------------------------------- containers
// per-launch HIP-event profiler (off by default): one (start, stop) event pair per bracket on the launch stream
struct Prof {
    enum { MAXEV = 65536 };
    bool on = false;
    std::vector<hipEvent_t> ev;
    std::vector<int> cls;
    std::vector<double> flops;
    int used = 0;
    ~Prof() {
        for (auto e : ev) (void)hipEventDestroy(e);
    }
    void clear() {
        used = 0;
        cls.clear();
        flops.clear();
    }
    // One launch site: start event, launch() -- which issues the launch(es) on s and returns their status (hipError_t or an F5 code) --,
    // stop event.  With the profiler off it is launch() alone.  The bracket is closed on every path, so a failed launch cannot leave
    // a record open (end() drops every later record once begins and ends stop pairing up).
    template <typename F> auto timed(int c, hipStream_t s, double fl, F&& launch) -> decltype(launch()) {
        begin(c, s, fl);
        const auto rc = launch();
        end(s);
        return rc;
    }
    template <typename F> auto timed(int c, hipStream_t s, F&& launch) -> decltype(launch()) { return timed(c, s, 0.0, launch); }

private:
    void begin(int c, hipStream_t s, double fl) {
        if (!on || used + 2 > MAXEV) return;
        while ((int)ev.size() < used + 2) {
            hipEvent_t e;
            if (hipEventCreate(&e) != hipSuccess) return;
            ev.push_back(e);
        }
        (void)hipEventRecord(ev[used], s);
        cls.push_back(c);
        flops.push_back(fl);
    }
    void end(hipStream_t s) {
        if (!on || used + 2 > MAXEV || (int)ev.size() < used + 2 || (int)cls.size() * 2 != used + 2) return;
        (void)hipEventRecord(ev[used + 1], s);
        used += 2;
    }
};
enum { PC_GEMM = 0, PC_ATTN = 1, PC_LN = 2, PC_CONV = 3, PC_MISC = 4, PC_TEXT = 5, PC_TIME = 6 };

// --------------------------------------------------------------------------------------- packed weights
template <typename T> struct LinW {
    T* w = nullptr;      // [N, ldw]; null where q holds the weight
    float* b = nullptr;  // [N] or null
    int N = 0, K = 0, ldw = 0;
    Rows8 q;             // F5_PREC_F8 (the four block GEMMs): e4m3 codes [N, ldw] and one e8m0 scale byte per output channel
    // the packed operand's bytes, whichever form holds it (the LayerNorm launches prefetch them)
    const char* bytes() const { return q ? reinterpret_cast<const char*>(q.codes) : reinterpret_cast<const char*>(w); }
    size_t nbytes() const { return (size_t)N * ldw * (q ? 1 : sizeof(T)); }
};
// The A operand of a backbone GEMM as its producer left it: rows of T [rows, K] (pre-split f32 rows under F5_PREC_F16X3), or
// (F5_PREC_F8, from the AdaLN LayerNorm) e4m3 rows.
template <typename T> struct ARows {
    T* p = nullptr;
    Rows8 q;
    ARows(T* rows) : p(rows) {}
    ARows(const Rows8& rows8) : q(rows8) {}
};

// One stream's weights of a block: q / k / v fused, out-projection, feed-forward pair
template <typename T> struct StreamW {
    LinW<T> qkv, out, ff1, ff2;
    float *qn = nullptr, *kn = nullptr;   // F5_OPT_QK_RMSNORM: gains of the RMSNorm on q / k [64]
};
template <typename T> struct BlockW {
    StreamW<T> x;                      // the only stream of the DiT / UNetT; the MMDiT's audio stream
    // MMDiT: the text stream's own weights (to_q_c / to_k_c / to_v_c fused, to_out_c, ff_c, c_q_norm / c_k_norm); the last,
    // context_pre_only block has neither c.out nor c.ff1 / c.ff2
    StreamW<T> c;
    LinW<T> skip;                      // UNetT concat projection (no bias)
    float* norm1_g = nullptr;          // UNetT RMSNorm gains
    float* norm2_g = nullptr;
};
// One stream's activation buffers in Work<T>: the f32 residual stream, its normed rows (the A operand of the QKV and FF1 GEMMs), the FF
// hidden rows and the out-projection's operand.  DiT / UNetT and the MMDiT's audio stream: w.x, w.xn, w.ffh and w.ao (MMDiT: w.mm_aox);
// the MMDiT's text stream: w.mm_c, w.mm_cn, w.mm_ffc, w.mm_aoc.
template <typename T> struct StreamBuf {
    float* x;
    ARows<T> xn;
    T *ffh, *ao;
};

struct TextBlockW {
    float *dwk = nullptr, *dwb = nullptr, *lnw = nullptr, *lnb = nullptr, *gamma = nullptr, *beta = nullptr;
    LinW<float> pw1, pw2;
};

template <typename T> struct Packed {
    LinW<float> time0, time2, mod;  // mod: stacked AdaLN linears [(6*depth+2)*D, D]
    float* E = nullptr;             // text embedding table
    std::vector<TextBlockW> tblocks;
    LinW<T> in_proj;
    T* conv_w[2] = {nullptr, nullptr};
    float* conv_b[2] = {nullptr, nullptr};
    int conv_kp = 0;
    std::vector<BlockW<T>> blocks;
    LinW<T> proj_out;
    LinW<T> long_skip;             // F5_OPT_LONG_SKIP: Linear(2 D -> D, no bias) over [x | residual] (dit.py:205,323-324)
    LinW<float> long_skip_f;       // ... and its split-planar f32 copy for F5_PREC_F16P (the operand is the raw stream)
    // F5_PREC_F16P: split-planar f32 copies of the input / output layers' weights (gemm2.h GemmOperands::WSplit / AWSplit, convpos.h SPLIT)
    LinW<float> in_proj_f, proj_out_f;
    float* conv_w_f[2] = {nullptr, nullptr};
    int conv_kp_f = 0;
    float* norm_out_g = nullptr;  // UNetT
    // aux tables
    float *rope_cos = nullptr, *rope_sin = nullptr, *time_freqs = nullptr, *text_pos = nullptr;
    float* rope_frag = nullptr;   // rope_cos / rope_sin in the QKV epilogue's fragment order (rope_frag_kernel)
    int text_pos_rows = 0;
};

// One adaptable tensor of an engine built with F5_OPT_ADAPTERS (registered by finalize_t as it packs): the state-dict name, the
// shape a put must match, and the "restore" descriptor -- fp32 master -> packed destination(s) -- an adapter's own descriptor starts from.
struct AdaptTarget {
    std::string name;
    std::vector<int64_t> shape;
    bool lowrank = false;   // takes a low-rank pair (else: replaceable in full)
    MergeDesc base{};
};
struct f5_adapter {
    f5_engine* eng = nullptr;     // null once the engine is gone
    unsigned gen = 0;             // the engine's adapt_gen when the adapter was created (a later f5_finalize makes it stale)
    MergeDesc* table = nullptr;   // device [targets]: the descriptors of the slots this adapter touches
    std::map<int, std::vector<void*>> bufs;   // slot -> the device copies (A, B or the replacement tensor) its descriptor points to
    ~f5_adapter() {
        for (auto& kv : bufs)
            for (void* p : kv.second) (void)hipFree(p);
        if (table) (void)hipFree(table);
    }
};

// Runtime switches: read once from the environment, in f5_create (engine.hip read_switches; the table in INTEGRATION.md).
struct Switches {
    bool graphs = true;            // F5_HIP_GRAPH=0: launch the sample() body eagerly
    // The conditional and unconditional halves of a CFG forward are independent until the Euler update: run them as two
    // concurrent kernel chains (second stream, fork/join events) so that one chain's launch ramps / drains overlap
    // the other chain's main loops.  Opt-in with F5_SPLIT_CFG=1: 35.4 ms as two eager chains, 35.2 ms as a two-branch
    // hipGraph, against 34.4 ms packed.  It steps the whole batch per half, on padded rows.
    bool split_cfg = false;
    bool pack_rows = true;         // F5_PACK_ROWS=0: attn_mask_enabled DiT batches on padded rows (no RowPack)
    long chunk_rows = 0;           // F5_CHUNK_ROWS: fixed row budget of one backbone call inside sample(); 0: unset (chunk_utts)
    bool weight_prefetch = true;   // F5_WEIGHT_PREFETCH=0: the LayerNorm launches do not prefetch the weights of the GEMMs behind them
    // Diagnostic (F5_X3_ABLATE=<bitmask>, F5_PREC_F16X3 only; tools/x3_ablate.py): contraction classes run with plain f16 products
    // (hi x hi only) instead of the three split products: 1 QKV, 2 attention K Q^T, 4 attention V^T P^T, 8 out-proj, 16 FF1, 32 FF2,
    // 64 input projection, 128 conv position embedding, 256 output projection
    int x3_ablate = 0;
    // F5_PREC_F16X3 attention: both products (K Q^T, V^T P^T) as PLAIN f16 products on the split operands' hi halves -- measured harmless
    // (tools/x3_ablate.py: DiT C2 1.10e-5 -> 1.01e-5, E2-TTS UNetT 1.7e-5 -> 5.2e-5; every GEMM class costs ~1e-3 there) and 7-9 % of
    // the f16x3 step.  F5_X3_ATTN_SPLIT=1 restores the three split products (and lets F5_X3_ABLATE bits 2 / 4 select).
    bool x3_attn_split = false;
    int x3_attn_hi() const { return x3_attn_split ? (x3_ablate >> 1) & 3 : 3; }
    // F5_LEN_BUCKET=<granule> / f5_set_length_buckets: length-bucketed sample() graphs.  0 (the default): off.  Else a multiple of 8 in
    // [8, 1024]: an eligible sample() call (bucket_eligible, engine_impl.h) is planned at N rounded up to the granule and its true
    // length reaches the kernels through the device tables of RowPack, so one captured graph serves every N of a bucket.
    int len_bucket = 0;
    // F5_STORE_WT=<mask of F5_WT_*, f5_common.h>: which classes of block kernel store write-through where a forward runs at <= 4,096 rows
    // (FwdCtx::wt).  Results do not depend on it.  The default: the classes that paid on their own at C2.
    int store_wt = F5_WT_DEFAULT;
    // f5_set_isolated_rows (off by default; no environment variable): f5_sample_items and f5_sample_span run on the packed body with each
    // row's own length in the device tables -- every row as if it were alone in the batch, whatever attn_mask_enabled says -- and, with
    // len_bucket on, at N's bucket ceiling.  A call that cannot keep that promise is refused (isolated_ceiling, engine_impl.h).
    bool isolated_rows = false;
};
inline bool valid_len_bucket(long g) { return g == 0 || (g >= 8 && g <= 1024 && g % 8 == 0); }

// HIP graphs of whole sample() bodies (one per problem signature): ~2600 launches per utterance become one
// hipGraphLaunch, so the host (shared, sometimes slow) can never be the bottleneck of the ODE loop.  A signature is
// captured the second time it is seen: its first call runs eagerly and marks it warm (f5_prepare_sample captures ahead of
// the first call instead).  The cache holds `capacity` entries, oldest out first: 16, or as many as f5_prepare_sample was
// asked to keep ready, MAX_CAPACITY at most.
// sample() returns without a host sync, so the launch of an entry may still be in flight when the entry is pushed out: every launch records
// the entry's event on the caller's stream (launched), and evict waits for it before it destroys the exec.
struct GraphCache {
    enum { DEFAULT_CAPACITY = 16, MAX_CAPACITY = 64 };
    // done: recorded behind the entry's last launch (made by its first one; null for a graph that never launched, as f5_prepare_sample's)
    struct Entry { std::string key; hipGraph_t graph; hipGraphExec_t exec; hipEvent_t done; };
    // f5_graph_stats: sample() bodies captured, replayed and launched eagerly, and entries pushed out by a newer capture
    struct Stats { int captures = 0, replays = 0, eager = 0, evictions = 0; };
    Stats stats;
    size_t capacity = DEFAULT_CAPACITY;
    std::vector<Entry> graphs;
    std::vector<std::string> warm;      // signatures (without cache state) that have run eagerly once
    hipStream_t cap_stream = nullptr;
    bool disabled = false;              // a capture failed: stop trying (the user's switch is Switches::graphs)
    GraphCache() = default;
    GraphCache(const GraphCache&) = delete;   // owns HIP handles (f5_engine's destructor releases them)
    void clear() {
        while (!graphs.empty()) evict(0);
        warm.clear();
    }
    hipGraphExec_t find(const std::string& key) const {
        for (auto& g : graphs)
            if (g.key == key) return g.exec;
        return nullptr;
    }
    bool is_warm(const std::string& base_key) const { return std::find(warm.begin(), warm.end(), base_key) != warm.end(); }
    void mark_warm(const std::string& base_key) {
        if (!is_warm(base_key)) warm.push_back(base_key);
    }
    // Captures the launches of body(cap_stream) and instantiates them as *exec; the oldest of `capacity` entries makes room.  Capture is an
    // optimisation: when it fails the cache says so, *exec stays null (the caller launches eagerly) and no later call tries again.
    template <typename F> int capture(const std::string& key, F&& body, hipGraphExec_t* exec) {
        if (!cap_stream) HIPCHK(hipStreamCreateWithFlags(&cap_stream, hipStreamNonBlocking));
        hipGraph_t graph = nullptr;
        if (hipStreamBeginCapture(cap_stream, hipStreamCaptureModeRelaxed) != hipSuccess) {
            fprintf(stderr, "libf5hip: hipStreamBeginCapture failed (%s); continuing with eager launches\n",
                    hipGetErrorString(hipGetLastError()));
        } else {
            const int rc = body(cap_stream);
            const hipError_t ce = hipStreamEndCapture(cap_stream, &graph);
            if (rc == F5_OK && ce == hipSuccess && graph && hipGraphInstantiate(exec, graph, nullptr, nullptr, 0) == hipSuccess) {
                while (graphs.size() >= capacity) {
                    evict(0);
                    stats.evictions++;
                }
                graphs.push_back({key, graph, *exec, nullptr});
                stats.captures++;
                return F5_OK;
            }
            // (say so: the wall time doubles on a busy host)
            fprintf(stderr, "libf5hip: HIP graph capture of sample() failed (body rc %d, end-capture: %s, last: %s); "
                            "continuing with eager launches\n", rc, hipGetErrorString(ce), hipGetErrorString(hipGetLastError()));
            if (graph) (void)hipGraphDestroy(graph);
        }
        *exec = nullptr;
        disabled = true;
        return F5_OK;
    }
    // after hipGraphLaunch(exec, s): marks the end of that launch on s, for evict
    int launched(hipGraphExec_t exec, hipStream_t s) {
        for (auto& g : graphs) {
            if (g.exec != exec) continue;
            if (!g.done) HIPCHK(hipEventCreateWithFlags(&g.done, hipEventDisableTiming));
            HIPCHK(hipEventRecord(g.done, s));
            break;
        }
        return F5_OK;
    }
    void evict(size_t i) {
        if (graphs[i].done) {   // the entry's last launch may still be running
            (void)hipEventSynchronize(graphs[i].done);
            (void)hipEventDestroy(graphs[i].done);
        }
        if (graphs[i].exec) (void)hipGraphExecDestroy(graphs[i].exec);
        if (graphs[i].graph) (void)hipGraphDestroy(graphs[i].graph);
        graphs.erase(graphs.begin() + i);
    }
};

struct f5_engine {
    f5_config cfg{};
    int inner = 0, kin = 0, kin_pad = 0, modN = 0;
    bool io_split = false;     // F5_PREC_F16P: the f16 engine with its input / output layers as split-f16 products on f32 operands
    bool f8 = false;           // F5_PREC_F8: F5_PREC_F16P (io_split is set too) with e4m3 operands in the four GEMMs of every DiT block
    bool split16 = false;      // F5_PREC_F16X3: the f32 engine with the backbone GEMMs on the f16 pipe (gemm2.h GemmOperands::WSplit)
    Switches sw;
    WeightStore ws;
    std::vector<void*> owned;  // packed buffers
    Packed<float> pf;
    Packed<bf16_t> pb;
    Packed<f16_t> ph;
    bool finalized = false;
    Arena arena;
    Staging stage;
    Prof prof;
    int res_B = 0, res_N = 0, res_S = 0;
    // The unconditional text embedding (all filler tokens) depends only on the weights and the length: cache it across
    // sample() calls for the single-utterance case (the reference recomputes it every call, dit.py:244-269).
    // The buffer lives in the arena (Work::uc), so its lifetime and the invalidation of captured graphs follow every
    // other captured pointer; uc_N = -1 whenever the arena moves or the weights change.
    int uc_N = -1;
    GraphCache gc;
    // F5_SPLIT_CFG (SamplePlan::split): the side stream and the fork / join events, made by the first call that needs them
    hipStream_t side_stream = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    int res_nt = 0;
    float* mm_taps = nullptr;  // f5k_mmdit_taps (diagnostic): where f5_dit_forward copies the MMDiT's intermediates; sample() never does
    bool res_items = false;    // a per-item call has run: the arena plan carries Work::mod_rows and the it_* tables ...
    int res_U = 0;             // ... and this many time rows (the most distinct evaluation times a per-item call has had)
    // resident adapters (F5_OPT_ADAPTERS; adapter.hip)
    bool adapters_on = false;
    std::vector<AdaptTarget> targets;
    std::map<std::string, int> target_slot;
    MergeDesc* base_table = nullptr;     // device [targets] (in `owned`)
    f5_adapter* active = nullptr;
    std::vector<f5_adapter*> adapters;   // every live adapter bound to this engine
    unsigned adapt_gen = 0;
    void clear_graphs() { gc.clear(); }
    ~f5_engine() {
        for (f5_adapter* a : adapters) a->eng = nullptr;
        clear_graphs();
        if (gc.cap_stream) (void)hipStreamDestroy(gc.cap_stream);
        if (side_stream) (void)hipStreamDestroy(side_stream);
        if (ev_fork) (void)hipEventDestroy(ev_fork);
        if (ev_join) (void)hipEventDestroy(ev_join);
        for (void* p : owned) (void)hipFree(p);
    }
};

template <typename U> static int dev_alloc(f5_engine* e, U** out, size_t n) {
    void* p = nullptr;
    HIPCHK(hipMalloc(&p, std::max<size_t>(n * sizeof(U), 16)));
    e->owned.push_back(p);
    *out = reinterpret_cast<U*>(p);
    return F5_OK;
}
// ---------------------------------------------------------------------------------------------- workspace
template <typename T> struct Work {
    // per call
    float *tdev, *feat, *th, *temb, *st, *mod;   // tdev: the evaluation times (feature rows), then the grid (sample_body)
    int* lens;        // per-sample lengths, chunk-major: for each chunk of Bc utterances [Bc values][the same Bc values]
    int* lens_plain;  // the same lengths once, in utterance order (text encoder)
    int* row_start;   // RowPack: per chunk [2 Bc + 1] first packed row of every batch row (cond half, uncond half), last = rows
    int2* rowmap;     // RowPack: per chunk, packed row -> (batch row, position)
    float *step_cond, *text_c, *text_u, *tx_a, *tx_b, *tx_h1, *grn_part;
    float* uc;        // cached unconditional text embedding [res_N, text_dim] (f5_engine::uc_N)
    unsigned char* dummy;
    // per forward
    T* acat;
    float *h, *c1, *x, *pred;
    T *xn, *q, *k, *vt, *ao, *ffh;
    // F5_PREC_F8 (else empty): the A operand of the block GEMM about to run -- e4m3 codes at the pitch of its K, in rows carved for the
    // widest one, pitch = max(D, inner, F) -- and its row scale bytes [rows]
    Rows8 a8;
    T* cat2;         // UNetT concat buffer [rows, 2D]
    float* skips;    // UNetT skip stack
    float* pred_all; // UNetT proj_out over N+1 tokens
    // sample(): engine-owned copies of the call's inputs / outputs so that the captured graph has stable pointers
    float *in_cond, *y, *out_buf, *traj_buf;
    float* y_mid;     // F5_ODE_MIDPOINT: the state at the half step [B, N, mel]
    unsigned char* in_mask;
    long long* in_text;
    // f5_sample_items (carved once a per-item call has asked for them, f5_engine::res_items; else null): the time rows of one evaluation
    // gathered per batch row [2 B, modN | D], and the per-item tables -- grids [B, steps_max + 1], guidance [B], step counts [B] and
    // the row of every (evaluation, item) in the time path's output [evals * steps_max, B]
    float *mod_rows, *it_t, *it_cfg;
    int *it_steps, *it_idx;
    // MMDiT (carved for that backbone only; else null): the text stream c [2 B * nt, D] f32, its normed rows, the two dense halves of the
    // split attention output, c's FF hidden rows and the joint key lengths nt + len.  text_c / text_u hold [B, nt, D] there, and q / k /
    // ao / vt the joint sequence of nt + N positions.
    float* mm_c;
    T *mm_cn, *mm_aox, *mm_aoc, *mm_ffc;
    int* mm_lens;
    int Npad;
};

// Row packing of a padded batch.  With attn_mask_enabled (modules.py:501-506) the frames past a sample's own length
// influence nothing -- the text is embedded per sample (dit.py:247-258), the conv position embedding masks them
// (modules.py:187-192), they are masked as attention keys and zeroed as attention queries (modules.py:540-542) and every
// other op is row-wise -- so the backbone runs on the valid rows only, the engine-side equivalent of the reference's
// unpad_input + flash_attn_varlen_func (modules.py:510-531) and of the TRT runtime's remove_input_padding
// (f5_tts_trtllm.py:448-456).  Batch row b' owns rows row_start[b'] .. row_start[b'+1]-1 (its length rounded up to a
// multiple of 4, so that the transposed V^T stores stay 8-byte aligned); q / k / V^T keep their padded per-batch-row layout,
// so the attention kernel is unchanged apart from where it writes its output rows.  All launch geometry stays that of
// the PADDED batch and every kernel reads the row count from row_start[Bp] on the device: a captured graph does not
// depend on the lengths.  ODE state, cond and the trajectory stay padded; frames past a sample's length keep their
// initial value there (the reference lets them drift: nobody reads them).
struct RowPack {
    const int* row_start = nullptr;   // device int[Bp + 1]
    const int2* rowmap = nullptr;     // device int2[rows]
    const int* rows_dev = nullptr;    // = row_start + Bp
    double rows_host = 0, sq_host = 0;
    explicit operator bool() const { return row_start != nullptr; }
};

// What one sample() call decides before it launches anything (engine.hip plan_sample); upload_small, sample_body and the graph key
// read it, nothing re-derives it.  The ODE state of different utterances never interacts, so the batch is stepped in chunks of
// `chunk` utterances (chunk_utts).
struct SamplePlan {
    struct Chunk { int idx, u0, bc; double rows, sq; };   // number, first utterance, utterances; packed rows present and sum of squared lengths (host: FLOP counts, tile choice)
    int B = 0, N = 0, nt = 0, steps = 0, method = F5_ODE_EULER;
    float cfg_strength = 0.f;
    bool use_cfg = true, has_lens = false, want_traj = false;
    int halves = 2;       // batch rows per utterance in a backbone call: cond + uncond, or 1 without CFG
    int evals = 1;        // backbone evaluations per step (midpoint: 2)
    bool pack = false;    // RowPack: attn_mask_enabled DiT batches with lengths, unless F5_PACK_ROWS=0 or F5_SPLIT_CFG=1; every bucket plan; every isolated plan
    // Length bucket (Switches::len_bucket): N above is the bucket's ceiling -- arena layout, launch grids, the graph key -- and every
    // utterance has n_true <= N frames, which only the device tables (lens, lens_plain, row_start) and the copies around the body know.
    // nt is then the capacity of the text staging buffer (f5_engine::res_nt), filled with -1 behind the call's tokens.  0: no bucket.
    int n_true = 0;
    bool split = false;   // F5_SPLIT_CFG=1: the halves as two stream chains (DiT with CFG, profiler off); one chunk, no packing
    int chunk = 0;
    // f5_sample_items: per-item grids, guidance and step counts in device tables (Work::it_*).  steps is then the largest step count,
    // U the rows of the time path (the distinct evaluation times of the call), and cfg_strength is not read.  Never split; packed when
    // isolated (Switches::isolated_rows): has_lens is then set, U is the call's count rounded up to a power of two (the rows behind the
    // call's own repeat its last time; no index points at them), and with `bucket` N is the ceiling of the call's length bucket and nt
    // the capacity of the text staging buffer, as in a bucket plan of sample() -- but every utterance keeps its own length.
    bool items = false;
    int U = 0;
    bool bucket = false;
    std::vector<Chunk> chunks;
    // Where a chunk lives in the per-call tables.  Work::lens holds [bc][the same bc] per chunk whatever `halves` is; a chunk's
    // row_start table has halves * bc + 1 entries; rowmap is carved for 2 B rows of round_up(N, 4); state, cond and text are [B, N, *].
    int lens_at(const Chunk& k) const { return 2 * k.u0; }
    int row_start_at(const Chunk& k) const { return halves * k.u0 + k.idx; }
    size_t rowmap_at(const Chunk& k) const { return (size_t)2 * k.u0 * round_up(N, 4); }
    size_t frame_at(const Chunk& k) const { return (size_t)k.u0 * N; }
};

// ------------------------------------------------------------------------------------ shared host helpers (engine.hip)
int ensure_arena(f5_engine* e, int B, int N, int S);
// what plan_sample is told beside the batch's shape and lengths; the defaults are a plan that only lays out the length tables
struct PlanOptions {
    int chunk = 0;        // utterances per chunk; 0: chunk_utts decides (text_embed / forward: the whole batch as one chunk, both halves)
    int nt = 0, steps = 0, method = F5_ODE_EULER;
    float cfg_strength = 1.f;
    bool want_traj = false;
    int n_true = 0;       // > 0: a length-bucket plan -- N is the bucket's ceiling, every utterance has n_true frames and lens_host is ignored
    bool items = false;   // a per-item plan of U time rows (cfg_strength: 1 when any item is guided, else 0)
    int U = 0;
    bool isolated = false;   // a per-item plan on packed rows: lens_host holds every utterance's own length (never null) and N is the arena's
    bool bucket = false;     // ... and N is a length bucket's ceiling, nt the text staging capacity
    static PlanOptions whole_batch(int B) {
        PlanOptions o;
        o.chunk = B;
        return o;
    }
};
SamplePlan plan_sample(const f5_engine* e, int B, int N, const int32_t* lens_host, const PlanOptions& o);
std::string graph_key(const SamplePlan& p);
std::vector<float> time_table(const float* t_host, int steps, int method);
// The time rows of a per-item call: the evaluation times of every live item, walked evaluation-major and then item-major, deduplicated
// by f32 bit pattern in first-appearance order -- for a uniform batch exactly time_table's evaluation rows, in its order.
// idx [evals * steps_max][B]: the row of every (evaluation, item); a finished item points at row 0.
struct ItemTimeRows {
    std::vector<float> times;
    std::vector<int32_t> idx;
};
ItemTimeRows item_time_rows(const float* t_items, const int32_t* steps_items, int steps_max, int B, int method);
// the host tables of a per-item call, as upload_small sends them down
struct ItemTables {
    const float* t_items = nullptr;        // [B][steps + 1]
    const float* cfg_items = nullptr;      // [B]
    const int32_t* steps_items = nullptr;  // [B]
    const ItemTimeRows* rows = nullptr;    // (made from the three once they have passed their checks)
};
// One sampler call as the ABI hands it over.  f5_sample, f5_sample_ode, f5_sample_items and f5_sample_span each fill one; engine.hip
// checks it (check_sample_call) and EngineOps<T>::run_sample runs it.  Three things differ between the entry points, and only these:
struct SampleCall {
    // what every entry point has, in the order the entry points brace-initialise it
    const char* who;   // the entry point, for messages
    const float* cond;   // [B, cond_frames, mel]
    int cond_frames;
    const uint8_t* cond_mask;
    const int64_t* text;
    int nt;
    const int32_t* lens_host;
    int B, N;
    float* out;
    hipStream_t stream;
    int method;
    // 1. the times: one grid t_host [steps + 1] and one guidance strength for the batch, or (per_item) tables, steps being the largest count
    bool per_item = false;
    const float* t_host = nullptr;
    int steps = 0;
    float cfg_strength = 0.f;
    ItemTables items;
    // 2. the start state: y0 [B, N, mel], or (span) row rows_host[b] of prev_state [prev_B, prev_N, mel], -1 standing for y_new[b]
    bool span = false;
    const float* y0 = nullptr;
    const float *y_new = nullptr, *prev_state = nullptr;
    int prev_B = 0, prev_N = 0;
    const int32_t* rows_host = nullptr;   // [B]
    // 3. what comes back beside `out`: the trajectory [steps + 1, B, N, mel] (or nothing), or (span) the raw state [B, N, mel]
    float* traj = nullptr;
    float* state_out = nullptr;
};
PlanOptions plan_options(const SampleCall& c);   // the plan of a call at its own N and text length (a length bucket changes nt and n_true)

// Entry points of one operand precision T (float: exact-f32 MFMA; bf16_t / f16_t: 16-bit MFMA operands, f32 accumulate).
template <typename T> struct EngineOps {
    static int finalize(f5_engine* e, hipStream_t s);
    static size_t plan_bytes(const f5_engine* e, int B, int N, int S);
    static size_t work_plan(const f5_engine* e, int B, int N, int S, int call_B, int call_N, int64_t* main_off, int64_t* side_off);
    static int text_embed(f5_engine* e, const int64_t* text, int B, int nt, const int32_t* lens_host, int N, int drop_text,
                          float* out, hipStream_t s);
    static int forward(f5_engine* e, const float* x, const float* cond, const int64_t* text, int nt, const float* time_host,
                       const int32_t* lens_host, int B, int N, int cfg_infer, int drop_audio_cond, int drop_text, float* out,
                       hipStream_t s);
    static int flow_loss(f5_engine* e, const float* x1, const float* x0, const int64_t* text, int nt, const float* time_host,
                         const int32_t* lens_host, const int32_t* span_host, int B, int N, int drop_audio_cond, int drop_text, double* sq_sum,
                         int32_t* count, float* pred, float* cond, float* frame_err, hipStream_t s);
    static int run_sample(f5_engine* e, const SampleCall& c);
    static int prepare(f5_engine* e, int B, int n_min, int n_max, int nt_max, int steps, float cfg_strength, int method, bool want_traj);
};
extern template struct EngineOps<float>;
extern template struct EngineOps<bf16_t>;
extern template struct EngineOps<f16_t>;
