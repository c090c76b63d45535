"""CPU: the two references of the text encoder pin each other, and the inputs of tests/test_text_encoder_gpu.py can tell a
wrong text encoder from a right one.

1. tests/text_oracle.py (float64, one sample at a time) against oracle.f5_oracle.text_embed_batch / unett_text_embed run
   in float32, on every case of tests/text_cases.py and both drop_text values, to float32 rounding:

       |oracle32 - ref64| <= 2^-23 * (n_max + 16 * layers * max|ref64|)          (exact without conv layers)

   n_max * 2^-23 is what the float32 position table can be off by: the angle n * f_j carries the relative rounding of f_j
   and of the product, so its absolute error grows with the row (5e-4 at row 4095) and reaches the output with a gain of
   about one.  The second term allows every block 16 ulp at the output's largest magnitude for its own arithmetic: seven
   taps, a LayerNorm, two GEMMs of K <= 4096 with sqrt(K)-ish growth, and the GRN.  The formula was written from the
   number formats; the errors measured against it are 3 to 15 times smaller.  A structural disagreement is far larger:
   the gentlest one below (tanh GELU) moves the output by 1e-3, the others by 0.2 to 14.

2. Every mutation of text_oracle.MUTATIONS moves the float64 reference by at least 20 x the bound of at least one case
   (the bound the GPU test holds the kernels to).  This is a check on the inputs, in the reference alone.
"""
import pytest
import torch

import text_cases as T
from text_oracle import MUTATIONS, pos_table64

DROPS = (False, True)


@pytest.mark.parametrize("name", [c.name for c in T.CASES])
def test_float64_reference_agrees_with_float32_oracle(name):
    c = T.CASE[name]
    for drop in DROPS:
        ref, o32 = T.reference(name, drop), T.oracle32(name, drop)
        assert o32.dtype == torch.float32 and ref.dtype == torch.float64 and o32.shape == ref.shape == (c.B, c.N, c.text_dim or 100)
        err, top = (o32.double() - ref).abs().max().item(), ref.abs().max().item()
        n_max = min(c.N, 4096) - 1
        tol = 2.0 ** -23 * (n_max + 16 * c.layers * top) if c.layers else 0.0
        print(f"[text refs] {name} drop_text={int(drop)}: |oracle32 - ref64| {err:.3e} (tolerance {tol:.3e}, max |ref| {top:.2f})")
        assert err <= tol
        assert torch.equal(o32 == 0, ref == 0), "the two references disagree about which elements are exactly zero"


def test_case_table_reaches_the_edges_it_claims():
    """The shape edges the cases are there for, checked on the inputs themselves."""
    c = T.CASE["up_ratios"]
    text = T.text_for(c)
    valid = [(text[b, :min(c.nt, L)] != -1).sum().item() for b, L in enumerate(c.lens)]
    assert valid == [12, 12, 12, 1] and [L % v for L, v in zip(c.lens, valid)] == [0, 0, 0, 0] and c.lens[2] == valid[2]
    assert T.CASE["up_rem2"].N % 12 == 2
    c = T.CASE["up_all_filler"]
    assert (T.text_for(c)[1] == -1).all() and not T.reference(c.name, False)[1].any()
    c = T.CASE["d64_l4_fillers"]
    text = T.text_for(c)
    assert (text[1] == -1).all() and (text[0, 5:8] == -1).all() and text[0, 4] != -1 and text[0, 8] != -1
    assert c.lens[0] == c.N and 16 > c.lens[1] % 16 > 0 and c.lens[2] < 7 and (c.B * c.N) % 4 and c.N % 16
    c = T.CASE["d100_l1_trunc"]
    assert c.nt > c.N and (c.text_dim or 100) % 32 and c.lens[1] < 7
    assert T.CASE["u64_l1_clamp"].N > 4096 and not T.CASE["u64_l1_clamp"].mask_padding
    for c in T.CASES:      # drop_text changes every case's output: both values are worth running
        assert not torch.equal(T.reference(c.name, False), T.reference(c.name, True)), c.name


def test_position_table_float64():
    t = pos_table64(8, 5)
    n = torch.arange(5, dtype=torch.float64)
    for j in range(4):
        f = 10000.0 ** (-2 * j / 8)
        assert torch.allclose(t[:, j], torch.cos(n * f), rtol=0, atol=1e-15) and torch.allclose(t[:, 4 + j], torch.sin(n * f), rtol=0, atol=1e-15)
    assert torch.equal(pos_table64(8, 4, first=1), t[1:])


@pytest.mark.parametrize("mutate", MUTATIONS)
def test_inputs_discriminate(mutate):
    """The mutated float64 reference leaves the right one by >= 20 x the case's bound on at least one case."""
    seen = []
    for c in T.CASES:
        for drop in DROPS:
            move = (T.reference(c.name, drop, mutate) - T.reference(c.name, drop)).abs().max().item()
            b = T.bound(c.name, drop)[0]
            if move >= 20 * b:
                seen.append(f"{c.name}/drop={int(drop)}: moves {move:.2e} = {move / b:.0f} x bound {b:.2e}")
    print(f"[text mutation] {mutate}: seen by {len(seen)} of {2 * len(T.CASES)} runs; " + "; ".join(seen[:4]))
    assert seen, f"no case tells the mutation {mutate!r} from the right text encoder"
