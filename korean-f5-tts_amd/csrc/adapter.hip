// Resident adapters: the f5_adapter_* / f5_set_adapter entry points of include/f5_hip.h (kernel: adapter.h; the table of
// adaptable tensors is recorded by finalize_t, engine_impl.h reg_target).
#include "engine_types.h"

static int live_engine(f5_adapter* a, f5_engine** out) {
    if (!a) return fail(F5_EINVAL, "null adapter");
    f5_engine* e = a->eng;
    if (!e || a->gen != e->adapt_gen || !e->finalized)
        return fail(F5_ESTATE, "the adapter's engine has been destroyed or finalized again: create a new adapter");
    *out = e;
    return F5_OK;
}

extern "C" int f5_adapter_create(f5_engine* e, f5_adapter** out) {
    if (!e || !out) return fail(F5_EINVAL, "f5_adapter_create: null argument");
    if (e->cfg.backbone == F5_BACKBONE_MMDIT) return fail(F5_EINVAL, "f5_adapter_create: resident adapters are built for the DiT backbone, not the MMDiT");
    if (!e->adapters_on) return fail(F5_ESTATE, "f5_adapter_create: the engine was created without F5_OPT_ADAPTERS");
    if (!e->finalized) return fail(F5_ESTATE, "f5_adapter_create: f5_finalize has not been called");
    f5_adapter* a = new f5_adapter();
    if (hipMalloc((void**)&a->table, std::max<size_t>(e->targets.size(), 1) * sizeof(MergeDesc)) != hipSuccess) {
        a->table = nullptr;
        delete a;
        return fail(F5_ENOMEM, "f5_adapter_create: hipMalloc of the descriptor table failed");
    }
    a->eng = e;
    a->gen = e->adapt_gen;
    e->adapters.push_back(a);
    *out = a;
    return F5_OK;
}

extern "C" int f5_adapter_destroy(f5_adapter* a) {
    if (!a) return F5_OK;
    if (f5_engine* e = a->eng) {
        if (e->active == a) return fail(F5_ESTATE, "f5_adapter_destroy: the adapter is active (f5_set_adapter another one, or NULL, first)");
        e->adapters.erase(std::remove(e->adapters.begin(), e->adapters.end(), a), e->adapters.end());
    }
    (void)hipDeviceSynchronize();   // a switch that reads this adapter's buffers may still be in flight
    delete a;
    return F5_OK;
}

static std::string shape_str(const int64_t* shape, int ndim) {
    std::string s;
    for (int i = 0; i < ndim; ++i) s += (i ? ", " : "") + std::to_string(shape[i]);
    return s;
}

// the slot of `name` for a put: engine alive, adapter not active, name known and of the requested kind
static int put_slot(f5_adapter* a, const char* name, bool lowrank, const char* fn, f5_engine** eo, int* slot) {
    CHK(live_engine(a, eo));
    if (!name) return fail(F5_EINVAL, "%s: null name", fn);
    f5_engine* e = *eo;
    if (e->active == a) return fail(F5_ESTATE, "%s('%s'): the adapter is active (f5_set_adapter another one, or NULL, first)", fn, name);
    auto it = e->target_slot.find(name);
    if (it == e->target_slot.end() || e->targets[it->second].lowrank != lowrank)
        return fail(F5_EINVAL, lowrank ? "%s: '%s' does not take a low-rank pair (adaptable: transformer_blocks.<i>.attn.{to_q,to_k,to_v,to_out.0}.weight, "
                                         "input_embed.proj.weight)"
                                       : "%s: '%s' cannot be replaced in full (replaceable: the text_embed.* tensors)", fn, name);
    *slot = it->second;
    return F5_OK;
}

// installs the descriptor and the buffers it points to for one slot (replacing an earlier put of the same name)
static int install(f5_adapter* a, int slot, const MergeDesc& d, std::vector<void*>&& bufs, hipStream_t s) {
    if (hipMemcpyAsync(a->table + slot, &d, sizeof(MergeDesc), hipMemcpyHostToDevice, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) {
        for (void* p : bufs) (void)hipFree(p);
        return fail(F5_EHIP, "adapter descriptor upload failed: %s", hipGetErrorString(hipGetLastError()));
    }
    auto it = a->bufs.find(slot);
    if (it != a->bufs.end())
        for (void* p : it->second) (void)hipFree(p);
    a->bufs[slot] = std::move(bufs);
    return F5_OK;
}

extern "C" int f5_adapter_put_lora(f5_adapter* a, const char* name, const void* A, const int64_t* a_shape, int32_t a_ndim, const void* B,
                                   const int64_t* b_shape, int32_t b_ndim, float scale, f5_stream stream) {
    f5_engine* e = nullptr;
    int slot = -1;
    CHK(put_slot(a, name, true, "f5_adapter_put_lora", &e, &slot));
    const AdaptTarget& t = e->targets[slot];
    if (!a_shape || !b_shape) return fail(F5_EINVAL, "f5_adapter_put_lora('%s'): null argument", name);
    if (a_ndim != 2 || b_ndim != 2)
        return fail(F5_EINVAL, "f5_adapter_put_lora('%s'): A and B must be matrices (A [rank, %d], B [%d, rank])", name, t.base.in, t.base.out);
    const int64_t rank = a_shape[0];
    if (rank < 1 || rank > 128) return fail(F5_EINVAL, "f5_adapter_put_lora('%s'): rank %lld outside 1 .. 128", name, (long long)rank);
    if (a_shape[1] != t.base.in || b_shape[0] != t.base.out || b_shape[1] != rank)
        return fail(F5_EINVAL, "f5_adapter_put_lora('%s'): A [%s] / B [%s] do not fit the weight [%d, %d] (A [rank, %d], B [%d, rank])", name,
                    shape_str(a_shape, 2).c_str(), shape_str(b_shape, 2).c_str(), t.base.out, t.base.in, t.base.in, t.base.out);
    if (!A || !B) return fail(F5_EINVAL, "f5_adapter_put_lora('%s'): null argument", name);
    hipStream_t s = (hipStream_t)stream;
    const size_t na = (size_t)rank * t.base.in, nb = (size_t)t.base.out * rank;
    float *dA = nullptr, *dB = nullptr;
    if (hipMalloc((void**)&dA, na * sizeof(float)) != hipSuccess || hipMalloc((void**)&dB, nb * sizeof(float)) != hipSuccess) {
        if (dA) (void)hipFree(dA);
        return fail(F5_ENOMEM, "f5_adapter_put_lora('%s'): hipMalloc failed", name);
    }
    std::vector<void*> bufs{dA, dB};
    if (hipMemcpyAsync(dA, A, na * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess ||
        hipMemcpyAsync(dB, B, nb * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess) {
        for (void* p : bufs) (void)hipFree(p);
        return fail(F5_EHIP, "f5_adapter_put_lora('%s'): copy failed: %s", name, hipGetErrorString(hipGetLastError()));
    }
    MergeDesc d = t.base;
    d.A = dA;
    d.B = dB;
    d.rank = (int)rank;
    d.scale = scale;
    return install(a, slot, d, std::move(bufs), s);
}

extern "C" int f5_adapter_put_tensor(f5_adapter* a, const char* name, const void* dev, const int64_t* shape, int32_t ndim, f5_stream stream) {
    f5_engine* e = nullptr;
    int slot = -1;
    CHK(put_slot(a, name, false, "f5_adapter_put_tensor", &e, &slot));
    const AdaptTarget& t = e->targets[slot];
    if (!dev || (!shape && ndim > 0) || ndim < 0) return fail(F5_EINVAL, "f5_adapter_put_tensor('%s'): bad arguments", name);
    if (std::vector<int64_t>(shape, shape + ndim) != t.shape)
        return fail(F5_EINVAL, "f5_adapter_put_tensor('%s'): shape [%s], the engine's is [%s]", name, shape_str(shape, ndim).c_str(),
                    shape_str(t.shape.data(), (int)t.shape.size()).c_str());
    hipStream_t s = (hipStream_t)stream;
    size_t n = 1;
    for (auto v : t.shape) n *= (size_t)v;
    float* dW = nullptr;
    if (hipMalloc((void**)&dW, std::max<size_t>(n * sizeof(float), 16)) != hipSuccess)
        return fail(F5_ENOMEM, "f5_adapter_put_tensor('%s'): hipMalloc failed", name);
    std::vector<void*> bufs{dW};
    if (hipMemcpyAsync(dW, dev, n * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess) {
        (void)hipFree(dW);
        return fail(F5_EHIP, "f5_adapter_put_tensor('%s'): copy failed: %s", name, hipGetErrorString(hipGetLastError()));
    }
    MergeDesc d = t.base;
    d.W = dW;
    return install(a, slot, d, std::move(bufs), s);
}

extern "C" int f5_set_adapter(f5_engine* e, f5_adapter* a, f5_stream stream) {
    if (!e) return fail(F5_EINVAL, "null engine");
    if (e->cfg.backbone == F5_BACKBONE_MMDIT) return fail(F5_EINVAL, "f5_set_adapter: resident adapters are built for the DiT backbone, not the MMDiT");
    if (!e->adapters_on) return fail(F5_ESTATE, "f5_set_adapter: the engine was created without F5_OPT_ADAPTERS");
    if (!e->finalized) return fail(F5_ESTATE, "f5_set_adapter: f5_finalize has not been called");
    if (a) {
        f5_engine* ae = nullptr;
        CHK(live_engine(a, &ae));
        if (ae != e) return fail(F5_EINVAL, "f5_set_adapter: the adapter belongs to another engine");
    }
    if (a == e->active) return F5_OK;
    hipStream_t s = (hipStream_t)stream;
    // jobs: restore what the active adapter touched and the new one does not, then everything the new one touches
    std::vector<unsigned short> jobs;
    if (e->active)
        for (auto& kv : e->active->bufs)
            if (!a || !a->bufs.count(kv.first)) jobs.push_back((unsigned short)kv.first);
    if (a)
        for (auto& kv : a->bufs) jobs.push_back((unsigned short)(kv.first | MERGE_TABLE_BIT));
    for (size_t j0 = 0; j0 < jobs.size(); j0 += MERGE_MAXJ) {
        const int nj = (int)std::min<size_t>(MERGE_MAXJ, jobs.size() - j0);
        MergeJobs mj{};
        int tiles = 1;
        for (int j = 0; j < nj; ++j) {
            mj.slot[j] = jobs[j0 + j];
            tiles = std::max(tiles, merge_tiles(e->targets[jobs[j0 + j] & (MERGE_TABLE_BIT - 1)].base));
        }
        hipLaunchKernelGGL(adapter_merge_kernel, dim3(tiles, nj), dim3(256), 0, s, e->base_table, a ? a->table : e->base_table, mj);
        KCHK();
    }
    e->active = a;
    e->uc_N = -1;   // the text encoder may have changed: the cached unconditional text embedding is stale
    return F5_OK;
}
