"""What the store pattern of a GEMM epilogue costs (csrc/kapi_diag.hip::store_pattern_kernel): MFMA-fragment order (32 / 64 contiguous
bytes per row per instruction) against row-major full lines, bf16 and f32 (with and without reading the same addresses first).

    python tools/store_pattern.py            the many-row shapes, plain stores
    python tools/store_pattern.py policy     the 2,048-row outputs of a C2 block, per store policy (plain / write-through sc1 / nt) and
                                             per-lane width, 60 back-to-back launches each: the write-back of what a launch leaves dirty
                                             in L2 is inside the per-launch time (store_policy_kernel)
"""
import ctypes as C, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from f5_tts_amd import _lib
lib = _lib.load()
s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
torch.zeros(1, device="cuda:0")
fn = lib.f5x_store_pattern_probe
fn.restype = C.c_int32
fn.argtypes = [C.c_int32] * 7 + [C.POINTER(C.c_float), C.c_void_p]


def run(m, n, mode, rd, policy, mi, iters):
    us = C.c_float(0)
    rc = fn(m, n, mode, rd, policy, mi, iters, C.byref(us), s)
    return us.value if rc == 0 else float("nan")


if "policy" in sys.argv[1:]:
    names = {0: "16-bit fragment order,  8 B/lane, 32-B pieces", 4: "16-bit fragment order, 16 B/lane, 64-B pieces",
             2: "f32 fragment order,    16 B/lane, 64-B pieces", 5: "16-bit LN row order,    8 B/lane", 6: "16-bit LN row order,   16 B/lane"}
    print("rows x cols  pattern                                         MB     plain  write-through        nt   (us per launch, 60 back to back)")
    for (m, n) in ((2048, 1024), (2048, 2048), (2048, 3072)):
        for mode in (0, 4, 2, 5, 6):
            for rep in range(2):   # twice: the spread of the probe itself
                us = [run(m, n, mode, 0, pol, 2, 60) for pol in (0, 1, 2)]
                mb = m * n * (4 if mode == 2 else 2) / 1e6
                print(f"{m}x{n}  {names[mode]}  {mb:5.1f}  {us[0]:8.2f}  {us[1]:13.2f}  {us[2]:8.2f}", flush=True)
    sys.exit(0)

names = {0: "bf16 fragment order (16 rows x 32 B)", 1: "bf16 row-major (8 rows x 128 B)", 2: "f32 fragment order (16 rows x 64 B)", 3: "f32 row-major (4 rows x 256 B)"}
for (m, n) in ((32768, 1024), (32768, 2048), (32768, 3072), (16384, 1024)):
    for mode in (0, 1, 2, 3):
        for rd in ((0,) if mode < 2 else (0, 1)):
            us = run(m, n, mode, rd, 0, 0, 20)
            b = m * n * (2 if mode < 2 else 4) * (2 if rd else 1)
            print(f"{m}x{n} {names[mode]}{' read+write' if rd else ' write'}: {us:7.1f} us  {b / us / 1e6:6.2f} TB/s", flush=True)
