"""Host model of the sample() graph cache, written from the words of include/f5_hip.h (the "graph cache" block, f5_reserve,
f5_set_length_buckets, f5_prepare_sample, f5_set_isolated_rows, f5_set_graph_capacity, f5_graph_stats) -- not from the C++.

Plain Python, nothing of the package: the model is fed the events an engine is fed and says, per call, which path the call takes
("eager", "capture" or "replay") and what f5_graph_stats reads afterwards.  The rules it holds:

  * a signature is captured the second time it is seen; the capturing call counts under `captures` only;
  * the cache holds `capacity` graphs and a capture into a full cache pushes out the oldest CAPTURE (first in, first out: a
    replay renews nothing); a signature that was pushed out is still warm, so its next sighting captures again;
  * a clear drops every graph, forgets what was warm and counts no eviction;
  * growth of the reserved batch, frames, steps or text length clears; so does the first per-item call and one with more time rows;
    all of these but the text length also forget the cached unconditional text embedding.  (The header lets a longer text keep
    it; the model forgets it there too, which no caller can tell apart: the call behind a clear is eager either way and leaves the
    embedding of its own N behind.)
  * set_length_buckets clears and puts the capacity back to 16; prepare only ever raises the capacity, captures without
    launching, evicts like any capture, and leaves its signatures warm (one that is pushed out captures again on its next call);
  * set_graph_capacity outside [16, 64] is refused; shrinking evicts the oldest captures at once;
  * where the unconditional embedding is cacheable -- B = 1, guidance on, no lens, no length bucket, an architecture whose
    embedding does not depend on the text -- the signature carries "|uc" (the call reads the kept embedding) or "|nouc", and a call
    that must store the embedding runs eagerly whatever is warm or captured.
"""
from __future__ import annotations

from dataclasses import dataclass

DEFAULT_CAPACITY, MAX_CAPACITY = 16, 64
COUNTERS = ("captures", "replays", "eager", "evictions")


@dataclass(frozen=True)
class Sig:
    """One f5_sample_ode call as the cache sees it.  lens: None (lens_host NULL), "equal" (every entry N) or "ragged"."""
    B: int
    N: int
    nt: int
    steps: int
    cfg: float
    lens: str | None = None
    traj: bool = True
    method: str = "euler"


@dataclass(frozen=True)
class ItemSig:
    """One f5_sample_items / f5_sample_span call: steps is the largest step count, U the distinct evaluation times of the call,
    guided whether any item has cfg >= 1e-5.  Grids and guidance values are not part of a per-item signature."""
    B: int
    N: int
    nt: int
    steps: int
    U: int
    guided: bool = True
    lens: str | None = None
    traj: bool = True
    method: str = "euler"


def uc_arch(arch: dict, backbone: str = "DiT") -> bool:
    """Whether the unconditional text embedding of this architecture depends on nothing but the weights and N."""
    if backbone not in ("DiT", "UNetT"):
        return False
    return not (arch.get("text_mask_padding", True) and arch.get("conv_layers", 0) > 0) and not arch.get("text_embedding_average_upsampling", False)


def _ceil_to(n: int, g: int) -> int:
    return -(-n // g) * g


class GraphCacheModel:
    def __init__(self, *, uc_arch: bool = True, graphs: bool = True, dit: bool = True):
        self.uc_arch, self.graphs_on, self.dit = uc_arch, graphs, dit
        self.capacity = DEFAULT_CAPACITY
        self.granule = 0
        self.isolated = False
        self.res = [0, 0, 0]          # reserved batch, frames, steps
        self.res_nt = 0
        self.res_items, self.res_U = False, 0
        self.uc_N = None              # the N the kept unconditional embedding was made for
        self.held: list[tuple] = []   # keys of the captured graphs, oldest capture first
        self.warm: set[tuple] = set()
        self.stats = dict.fromkeys(COUNTERS, 0)

    # ------------------------------------------------------------------------------------------- what clears
    def _clear(self):
        self.held.clear()
        self.warm.clear()

    def _reserve(self, B, N, S, *, nt=0):
        if nt > self.res_nt:
            self.res_nt = nt
            self._clear()
            self.uc_N = None
        grown = [max(a, b) for a, b in zip(self.res, (B, N, S))]
        if grown != self.res:
            self.res = grown
            self._clear()
            self.uc_N = None

    def _reserve_items(self, U):
        if not self.res_items or U > self.res_U:
            self.res_items, self.res_U = True, max(self.res_U, U)
            self._clear()
            self.uc_N = None

    # ------------------------------------------------------------------------------------------- events
    def reserve(self, B, N, S):
        self._reserve(B, N, S)
        return None, dict(self.stats)

    def set_length_buckets(self, granule):
        self.granule = granule
        self._clear()
        self.capacity = DEFAULT_CAPACITY
        return None, dict(self.stats)

    def set_isolated_rows(self, on):
        self.isolated = bool(on)
        return None, dict(self.stats)

    def set_graph_capacity(self, n):
        if not DEFAULT_CAPACITY <= n <= MAX_CAPACITY:
            raise ValueError(f"graph capacity {n}: expected {DEFAULT_CAPACITY} to {MAX_CAPACITY} graphs")
        self.capacity = n
        while len(self.held) > self.capacity:
            self._evict()
        return None, dict(self.stats)

    def reset_stats(self):
        self.stats = dict.fromkeys(COUNTERS, 0)

    def prepare(self, B, n_min, n_max, nt_max, steps, cfg, method="euler", traj=True):
        assert self.granule > 0 and self.graphs_on and self.dit, "f5_prepare_sample needs length buckets and graphs"
        g = self.granule
        c0, c1 = _ceil_to(n_min, g), _ceil_to(n_max, g)
        count = (c1 - c0) // g + 1
        if count > MAX_CAPACITY:
            raise ValueError(f"{count} buckets; the graph cache holds at most {MAX_CAPACITY}")
        self._reserve(B, c1, steps, nt=nt_max)
        self.capacity = max(self.capacity, count)
        for nc in range(c0, c1 + g, g):
            key = ("L", B, nc, steps, float(cfg), traj, method, "nouc")
            self.warm.add(key[:-1])   # prepared counts as seen
            if key not in self.held:
                self._capture(key)
        return None, dict(self.stats)

    def sample(self, s: Sig):
        bucket = self.granule > 0 and self.dit and s.lens != "ragged"
        Nc = _ceil_to(s.N, self.granule) if bucket else s.N
        self._reserve(s.B, Nc, s.steps, nt=s.nt)
        if bucket:   # the ceiling stands for N; neither the call's own length nor its text length is part of the signature
            base = ("L", s.B, Nc, s.steps, float(s.cfg), s.traj, s.method)
        else:
            base = ("X", s.B, s.N, s.nt, s.steps, float(s.cfg), s.lens is not None, s.traj, s.method)
        uc_ok = self.uc_arch and not bucket and s.B == 1 and s.lens is None and not s.cfg < 1e-5
        return self._call(base, uc_ok, s.N)

    def sample_items(self, s: ItemSig):
        iso = self.isolated
        bucket = iso and self.granule > 0
        Nc = _ceil_to(s.N, self.granule if bucket else 4) if iso else s.N
        U = s.U
        if iso:
            while U & (U - 1):
                U += U & -U
        halves = 2 if s.guided else 1
        self._reserve(0, 0, 0, nt=s.nt)
        self._reserve_items(U)
        self._reserve(s.B, Nc, s.steps)
        if iso:
            base = ("P", s.B, Nc, s.steps, U, halves, s.traj, s.method) + (() if bucket else (s.nt,))
        else:
            base = ("I", s.B, s.N, s.nt, s.steps, U, halves, s.lens is not None, s.traj, s.method)
        uc_ok = self.uc_arch and not iso and s.B == 1 and s.lens is None and s.guided
        return self._call(base, uc_ok, s.N)

    # ------------------------------------------------------------------------------------------- the three paths
    def _evict(self):
        self.held.pop(0)
        self.stats["evictions"] += 1

    def _capture(self, key):
        while len(self.held) >= self.capacity:
            self._evict()
        self.held.append(key)
        self.stats["captures"] += 1

    def _call(self, base, uc_ok, N):
        uc_hit = uc_ok and self.uc_N == N
        key = base + ("uc" if uc_hit else "nouc",)
        path = "eager"
        if self.graphs_on and not (uc_ok and not uc_hit):
            if key in self.held:
                path = "replay"
                self.stats["replays"] += 1
            elif base in self.warm:
                path = "capture"
                self._capture(key)
        if path == "eager":
            self.stats["eager"] += 1
            self.warm.add(base)
            if uc_ok and not uc_hit:
                self.uc_N = N
        return path, dict(self.stats)
