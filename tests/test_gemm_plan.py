"""CPU: launch_gemm's dispatch decision (plan_gemm, csrc/gemm_dispatch.h) seen through f5k_gemm_plan, which launches nothing.
The recorded grid (tests/golden/gemm_plan.json, tools/gemm_plan_record.py) pins every decision; a second, hand-typed table states
what the cost table and the comments of gemm_dispatch.h imply, independently of the code."""
import json
import os

import pytest

from conftest import GOLDEN

from gpu_util import k_gemm_plan

V1, RING, PP = 1, 2, 3   # kernel families: gemm.h, gemm2.h, gemm3.h
NIN = 12                 # inputs per row: elem_size, M, N, K, has_m_limit, m_hint, form, conv, pp_epi, force_cfg, env_cfg, env_n


@pytest.fixture(scope="module")
def rows():
    with open(os.path.join(GOLDEN, "gemm_plan.json")) as fh:
        out = []
        for r in json.load(fh):
            n = r[NIN]
            plan = None if n < 0 else [tuple(r[NIN + 1 + 4 * i:NIN + 5 + 4 * i]) for i in range(n)]
            assert len(r) == NIN + 1 + 4 * max(n, 0)
            out.append((tuple(r[:NIN]), plan))
        return out


def test_library_reproduces_the_recorded_plans(rows):
    assert len(rows) >= 1000
    bad = [(g, plan, k_gemm_plan(*g)) for g, plan in rows if k_gemm_plan(*g) != plan]
    assert not bad, f"{len(bad)} of {len(rows)} plans differ, first: {bad[0]}"


def test_fixture_covers_every_outcome_kind(rows):
    """A condition on the fixture: a shrunken grid cannot hide a branch of the dispatch."""
    plans = dict(rows)
    assert len(plans) == len(rows), "duplicate grid rows"

    def some(pred):
        return any(pred(dict(zip(("es", "M", "N", "K", "ml", "mh", "form", "conv", "pp", "force", "env", "env_n"), g)), p) for g, p in rows)

    def single(p, fam, tile):
        return p is not None and len(p) == 1 and p[0][:2] == (fam, tile)

    def variant(g, **kw):   # the plan of the row that differs from g in the named inputs only (KeyError: not in the grid)
        names = ("es", "M", "N", "K", "ml", "mh", "form", "conv", "pp", "force", "env", "env_n")
        return plans.get(tuple(kw.get(n, v) for n, v in zip(names, g)), "absent")

    auto = lambda i: i["force"] == -1 and i["env"] == -1
    for tile in (128128, 128064, 64064):
        assert some(lambda i, p: single(p, V1, tile)), f"no v1 plan at tile {tile}"
    for tile in (2, 8, 9, 10, 13):
        assert some(lambda i, p: auto(i) and single(p, RING, tile)), f"no automatic ring plan at tile {tile}"
    assert some(lambda i, p: auto(i) and single(p, PP, 20))
    assert some(lambda i, p: auto(i) and p == [])                                      # M <= 0: nothing to do
    for es, form in ((2, 0), (4, 2)):   # main + remainder, for both operand forms that have a ping-pong kernel
        assert some(lambda i, p: (i["es"], i["form"]) == (es, form) and p is not None and len(p) == 2 and p[0] == (PP, 20, 0, i["M"] - i["M"] % 256)
                    and p[1] == (RING, 8, i["M"] - i["M"] % 256, i["M"] % 256))
    # the pre-split 64x64 preference: fires (128x64 with W split alone, 64x64 with both split) / does not (128x64 stays)
    assert any(auto(dict(force=g[9], env=g[10])) and g[6] == 2 and single(p, RING, 8) and single(variant(g, form=1), RING, 9) for g, p in rows)
    assert some(lambda i, p: auto(i) and i["form"] == 2 and single(p, RING, 9))
    # m_hint changes the tile
    assert any(g[5] > 0 and p is not None and variant(g, mh=0) not in ("absent", None, p) for g, p in rows)
    # forced tiles: every id as itself, "v1", an id that names no tile, the ping-pong tile where no such kernel exists
    for tile in (2, 8, 9, 10, 13):
        assert some(lambda i, p: i["force"] == tile and single(p, RING, tile) and i["M"] > 64)
    assert some(lambda i, p: i["force"] == 20 and single(p, PP, 20))
    assert some(lambda i, p: i["force"] == -2 and p is not None and len(p) == 1 and p[0][0] == V1 and i["K"] % (128 // i["es"]) == 0)
    assert some(lambda i, p: i["force"] == 5 and single(p, RING, 8))
    for where in (lambda i: i["form"] == 1, lambda i: i["conv"] == 1, lambda i: i["es"] == 4 and i["form"] == 0, lambda i: i["pp"] == 0):
        assert some(lambda i, p: i["force"] == 20 and where(i) and i["K"] % (128 // i["es"]) == 0 and (i["es"] == 4 or not i["form"]) and p is None)
    # the environment override: taken, taken for one N only, the ping-pong tile only where the plan may choose it
    assert some(lambda i, p: i["env"] == 13 and i["env_n"] == 0 and single(p, RING, 13))
    assert some(lambda i, p: i["env"] == 2 and i["env_n"] == 1024 and i["N"] != 1024 and not single(p, RING, 2))
    assert some(lambda i, p: i["env"] == 20 and single(p, PP, 20)) and some(lambda i, p: i["env"] == 20 and p and p[0][0] == RING)
    # every refusal
    ragged = lambda i: i["K"] % (128 // i["es"]) != 0
    for why in (lambda i: i["form"] and i["es"] == 4 and ragged(i), lambda i: i["form"] and i["es"] == 4 and i["force"] == -2 and not ragged(i),
                lambda i: i["conv"] and not i["form"] and ragged(i), lambda i: i["conv"] and not i["form"] and i["force"] == -2 and not ragged(i),
                lambda i: i["es"] == 2 and i["form"] and not ragged(i) and i["force"] != -2,
                lambda i: i["ml"] and not i["form"] and not i["conv"] and ragged(i),
                lambda i: i["ml"] and not i["form"] and not i["conv"] and i["force"] == -2 and not ragged(i)):
        assert some(lambda i, p: p is None and i["M"] > 0 and why(i))


# Typed in by hand from the cost table (us per round of 256 workgroups: 256x256 37.0, 256x128 21.0, 128x192 19.3, 128x128 14.5,
# 128x64 7.3, 64x64 4.0; ties keep the larger tile) and the comments of gemm_dispatch.h; not produced by running the code.
# (elem_size, M, N, K, has_m_limit, m_hint, form, force_cfg) -> plan.  16-bit cases: an epilogue that admits the ping-pong tile.
FACTS = [
    ((2, 2048, 3072, 1024, 0, 0, 0, -1), [(RING, 10, 0, 2048)]),      # one round of 128x192
    ((2, 2048, 1024, 1024, 0, 0, 0, -1), [(RING, 9, 0, 2048)]),
    ((2, 2048, 2048, 1024, 0, 0, 0, -1), [(RING, 2, 0, 2048)]),       # 14.5 against 14.6
    ((2, 16, 1024, 1024, 0, 0, 0, -1), [(RING, 8, 0, 16)]),
    ((4, 16, 1024, 1024, 0, 0, 0, -1), [(RING, 8, 0, 16)]),
    ((4, 16, 1024, 1024, 0, 0, 2, -1), [(RING, 8, 0, 16)]),
    ((2, 16384, 1024, 1024, 0, 0, 0, -1), [(PP, 20, 0, 16384)]),
    ((4, 16384, 1024, 1024, 0, 0, 0, -1), [(RING, 13, 0, 16384)]),    # no ping-pong for plain f32
    ((2, 16400, 1024, 1024, 0, 0, 0, -1), [(PP, 20, 0, 16384), (RING, 8, 16384, 16)]),
    ((2, 16400, 1024, 1024, 1, 0, 0, -1), [(RING, 13, 0, 16400)]),
    ((2, 16400, 1024, 1024, 1, 16384, 0, -1), [(PP, 20, 0, 16400)]),
    ((4, 2048, 1024, 1024, 0, 0, 2, -1), [(RING, 8, 0, 2048)]),       # the 64x64 preference: 512 tiles
    ((4, 2048, 2048, 1024, 0, 0, 2, -1), [(RING, 2, 0, 2048)]),
    ((4, 300, 100, 100, 0, 0, 0, -1), [(V1, 64064, 0, 300)]),
    ((4, 300, 100, 100, 1, 0, 0, -1), None),
    ((4, 300, 100, 100, 0, 0, 1, -1), None),
    ((4, 300, 100, 100, 0, 0, 2, -1), None),
]


@pytest.mark.parametrize("case,plan", FACTS, ids=[",".join(map(str, c)) for c, _ in FACTS])
def test_hand_derived_facts(case, plan):
    es, M, N, K, ml, mh, form, force = case
    assert k_gemm_plan(es, M, N, K, ml, mh, form, 0, 1, force) == plan
