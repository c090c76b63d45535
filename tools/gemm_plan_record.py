"""Records tests/golden/gemm_plan.json: launch_gemm's decision (f5k_gemm_plan, no GPU needed) over a grid of problems.
Each row is the twelve inputs of f5k_gemm_plan, then the number of launches (-1: refused), then four ints per launch.
usage: python tools/gemm_plan_record.py"""
import itertools
import json
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from gpu_util import k_gemm_plan

FORMS = ((2, 0), (4, 0), (4, 1), (4, 2))                 # (element size, operand form)
ROWS = ((0, 0), (1, 0), (1, 2048), (1, 16384))           # (device row count present, m_hint)
SHAPES = ((0, 1024), (16, 1024), (64, 4096), (300, 100), (2048, 1024), (2048, 2048), (2048, 3072), (4096, 1024), (4112, 1024),
          (16384, 1024), (16400, 1024), (16400, 3072))
RAGGED_K = ((300, 100), (2048, 1024), (2048, 2048))      # K = 100: no whole K-tile, the register-staged kernel's three tiles


def grid():
    for (es, form), pp, conv, (ml, mh) in itertools.product(FORMS, (1, 0), (0, 1), ROWS):       # the dispatch left to itself
        for (M, N), K in [(s, 1024) for s in SHAPES] + [(s, 100) for s in RAGGED_K]:
            yield (es, M, N, K, ml, mh, form, conv, pp, -1, -1, 0)
    for (es, form), pp, conv, ml, force in itertools.product(FORMS, (1, 0), (0, 1), (0, 1), (-2, 2, 8, 9, 10, 13, 20, 5)):   # forced
        for M, N, K in ((2048, 1024, 1024), (300, 100, 100)):
            yield (es, M, N, K, ml, 0, form, conv, pp, force, -1, 0)
    for (es, form), conv, env, env_n in itertools.product(FORMS, (0, 1), (2, 13, 20, 7), (0, 1024)):   # F5_GEMM_CFG / F5_GEMM_CFG_N
        for M, N in ((2048, 1024), (2048, 3072), (16400, 1024)):
            yield (es, M, N, 1024, 0, 0, form, conv, 1, -1, env, env_n)
    for form, K, force in itertools.product((1, 2), (1024, 100), (-1, -2, 20)):   # 16-bit rows have no split form
        yield (2, 2048, 1024, K, 0, 0, form, 0, 1, force, -1, 0)


def record(path):
    rows = []
    for g in grid():
        plan = k_gemm_plan(*g)
        rows.append(list(g) + ([-1] if plan is None else [len(plan)] + [v for l in plan for v in l]))
    with open(path, "w") as fh:
        fh.write("[\n" + ",\n".join(json.dumps(r, separators=(",", ":")) for r in rows) + "\n]\n")
    return len(rows)


if __name__ == "__main__":
    out = os.path.join(ROOT, "tests", "golden", "gemm_plan.json")
    print(record(out), "rows ->", out, os.path.getsize(out), "bytes")
