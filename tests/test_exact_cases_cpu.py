"""The exact-sum inputs of tests/test_kernels_exact_gpu.py, checked on the reference alone (no GPU): the inputs are good enough to see
a rounding mode, fp32 sums of their terms do not depend on the order, and the element-wise comparison catches - and locates - the
errors that the rel-L2 bounds of tests/test_kernels_gpu.py let through."""
import numpy as np
import pytest
import torch

import exact_cases as E
from exact_cases import BF16, F16, F32
from oracle import denoiser_oracle as O

CASES = E.reference_cases()
MIN_INEXACT, MIN_TIES = 0.05, 0.005


def _id(case):
    entry, shape, dt, special = case
    return f"{entry}-{'x'.join(map(str, shape))}-{E.DTYPE_NAMES[dt]}" + (f"-{special}" if special else "")


def rounding_shares(ref, out_dt):
    """share of reference values that the output type cannot hold, and share that lie exactly half-way between two neighbours"""
    got = E.expected(ref, out_dt).to(torch.float64).numpy()
    err = np.abs(ref - got)
    _, ex = np.frexp(ref)
    ulp = np.ldexp(1.0, ex - E.SIG_BITS[out_dt])
    return float(np.mean(err != 0)), float(np.mean((err != 0) & (2 * err == ulp)))


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_input_quality(case):
    """conditions on the INPUTS of every GPU case (not measurements of a kernel): the budget holds, the operands survive their storage
    type, the reference is exact in float32 and - for 16-bit outputs - at least 5 % of the reference values are not representable
    in the output type and at least 0.5 % are exact ties, without which an equality test could not tell round-to-nearest-even from
    truncation or from ties-away.  The shares are taken on the plain variant of a case (no ReLU, no mask): the masked variants
    compare a subset of the same values."""
    c = E.make_case(*case)
    if c.entry.startswith("dense"):
        E.assert_budget(c.ops); E.assert_budget(c.fwd_ops); E.assert_budget(c.dx_ops)
        assert E.survives_storage(c.x, c.dt) and E.survives_storage(c.w, F32) and E.survives_storage(c.dy, F16 if c.dt == F16 else F32)
        refs = [c.pred if c.entry == "dense_fwd" else c.dx]
        for r in (c.dw, c.db, 2 * c.dw, 2 * c.db, c.pred):
            E.expected(r, F32)
    else:
        E.assert_budget(c.ops)
        assert E.survives_storage(c.ops.a, c.dt) and E.survives_storage(c.ops.b, c.dt)
        if hasattr(c, "bias"):
            assert E.survives_storage(c.bias, F32)
        if hasattr(c, "prev"):
            assert E.survives_storage(c.prev, c.dt) and E.survives_storage(c.act, c.dt)
            assert (c.act > 0).any() and (c.act < 0).any() and (c.act == 0).any()
        refs = [c.ref] + ([c.ref + c.prev] if hasattr(c, "prev") else [])
        if c.out_dt == F32 and hasattr(c, "db"):
            E.expected(c.db, F32); E.expected(2 * c.db, F32); E.expected(2 * c.dw, F32)
    for r in refs:
        E.expected(r, c.out_dt)                      # asserts that float32 holds the reference exactly
        assert np.isfinite(r).all()
        if c.out_dt != F32:
            assert np.abs(r).max() < 65504
            inexact, ties = rounding_shares(r, c.out_dt)
            assert inexact >= MIN_INEXACT and ties >= MIN_TIES, (inexact, ties)


@pytest.mark.parametrize("case", E.special_cases(), ids=_id)
def test_special_inputs(case):
    """the {-1, 0, 1} grids of the fused bias gradients (every stored value exact in bf16), the fp16 overflow cases (1 % .. 50 % of
    the masked |gradient| at or above 65520, operands still fp16) and the grids without zero of the inf cases: budget, storage types
    and the precondition each of them exists for"""
    c = E.make_case(*case)
    E.assert_budget(c.ops)
    assert E.survives_storage(c.ops.a, c.dt) and E.survives_storage(c.ops.b, c.dt)
    if c.special == "pm1":
        g = E.dgrad_ref(c, 1, 0)
        assert np.abs(g).max() <= 256 and E.survives_storage(2 * g, BF16) and set(np.unique(c.dz)) == {-1.0, 0.0, 1.0} == set(np.unique(c.w))
    elif c.special == "overflow":
        ref = E.dgrad_ref(c, 1, 0)
        share = float(np.mean(np.abs(ref) >= 65520))
        assert 0.01 <= share <= 0.5 and share == c.overflow_share
        want = E.expected(ref, F16)
        assert int(torch.isinf(want).sum()) == int((np.abs(ref) >= 65520).sum()) and float(want[torch.isfinite(want)].abs().max()) <= 65504
    else:
        assert (c.ops.a != 0).all() and (c.ops.b != 0).all()
        E.expected(c.ref, F32)


@pytest.mark.parametrize("case", [("conv_fwd", E.SPLITK_SHAPE, BF16, None), ("conv_wgrad", (9, 4, 8, 64, 64), F16, None),
                                  ("dense_fwd", E.DENSE_SHAPE, F32, None)], ids=_id)
def test_float32_sums_do_not_depend_on_the_order(case):
    """the terms of 50 outputs, summed in float32 in 20 shuffled orders (one running sum: every prefix is a partial sum some tiling
    could form), always give the fp64 value"""
    c = E.make_case(*case)
    ref = c.pred if c.entry == "dense_fwd" else c.ref
    rng = np.random.default_rng(7)
    for _ in range(50):
        index = tuple(int(rng.integers(0, n)) for n in ref.shape)
        terms = c.terms_of(index)
        assert float(terms.sum()) == ref[index]
        for _ in range(20):
            acc = np.float32(0)
            for t in rng.permutation(terms).astype(np.float32):
                acc = np.float32(acc + t)
            assert float(acc) == ref[index], (index, float(acc), ref[index])


# ---- mutants ---------------------------------------------------------------------------------------------------------------------

GAP_SHAPE = (3, 32, 32, 3, 128)


def _truncate_bf16(ref):
    u = torch.tensor(ref, dtype=torch.float64).to(torch.float32).view(torch.int32)
    return ((u >> 16) << 16).view(torch.float32).to(torch.bfloat16)


def _ties_away_bf16(ref):
    t = torch.tensor(ref, dtype=torch.float64).to(torch.float32)
    u = t.view(torch.int32)
    tie = (u & 0xFFFF) == 0x8000
    return torch.where(tie, (((u >> 16) + 1) << 16).view(torch.float32), t).to(torch.bfloat16)


def _drop_corner_tap(x, w, b):
    """tap (1, 1) - the one that reads the corner pixel of the image - missing at the first output pixel of image 0"""
    ref = O.conv4s2_fwd(x, w, b)
    w2 = w.copy(); w2[1, 1] = 0
    ref[0, 0, 0] = O.conv4s2_fwd(x[:1], w2, b)[0, 0, 0]
    return ref


def _fails_with(got, want):
    with pytest.raises(AssertionError) as info:
        E.assert_elementwise_equal(got, want)
    return str(info.value)


def test_mutants_fail_and_are_located():
    """Six wrong outputs, each made from the oracle's own output, fail the element-wise comparison with a message that names where.

    The gap this closes, on test_conv4s2_fwd's own inputs (seeded normal draws, (3, 32, 32, 3, 128), bf16, bound 4e-3 rel-L2):
    the correctly rounded oracle lies 1.66e-3 from fp64, the TRUNCATED one 3.32e-3 and the one with the corner TAP DROPPED at one
    corner pixel 2.88e-3 - both pass today's bound (asserted below; other single taps at the four corners measure 2.9e-3 .. 1.0e-2, so
    some are caught and some are not); on exact-sum inputs both fail here."""
    c = E.make_case("conv_fwd", GAP_SHAPE, BF16)
    want = E.expected(c.ref, BF16)
    B, Ho, Wo, Cout = want.shape
    # 1. truncation instead of round-to-nearest-even
    msg = _fails_with(_truncate_bf16(c.ref), want)
    assert "shared: nothing" in msg
    # 2. ties away from zero
    away = _ties_away_bf16(c.ref)
    msg = _fails_with(away, want)
    u = torch.tensor(c.ref).to(torch.float32).view(torch.int32)
    flips = ((u & 0xFFFF) == 0x8000) & (((u >> 16) & 1) == 0)      # ties whose kept significand is even: nearest-even rounds them down
    assert int(flips.sum()) > 0 and f"{int(flips.sum())} of {want.numel()} elements differ" in msg
    assert torch.equal(away.view(torch.int16) != want.view(torch.int16), flips)
    assert f"  {tuple(int(v) for v in flips.nonzero()[0])}: " in msg                # the first index named is the first such tie
    # 3. one tap dropped at one corner pixel
    msg = _fails_with(E.expected(_drop_corner_tap(c.x, c.w, c.bias), BF16), want)
    assert "all in b = 0; all in h = 0; all in w = 0" in msg and "(0, 0, 0, " in msg
    # 4. the bias shifted by one column: every pixel, wherever neighbouring biases differ
    msg = _fails_with(E.expected(c.ref - c.bias + np.roll(c.bias, 1), BF16), want)
    assert "(0, 0, 0, " in msg and "shared: nothing" in msg
    # 5. one element wrong by one ulp
    one = want.clone()
    one.view(torch.int16)[1, 3, 5, 77] += 1
    msg = _fails_with(one, want)
    assert "1 of" in msg and "(1, 3, 5, 77)" in msg and "all in b = 1; all in h = 3; all in w = 5; all in c = 77" in msg
    # 6. a leak: 1e-3 of the neighbour channel added to the channels of the last 8-channel chunk (not an exact sum any more:
    #    rounded like a kernel would, through float32)
    leak = c.ref.copy()
    leak[..., 120:] += 1e-3 * c.ref[..., 119:-1]
    msg = _fails_with(torch.tensor(leak).to(torch.float32).to(torch.bfloat16), want)
    assert "all in c >= 120" in msg

    # today's inputs and metric let mutants 1 and 3 through
    rng = np.random.default_rng(1)
    rnd = lambda a: torch.tensor(a, dtype=torch.float64).to(torch.bfloat16).to(torch.float64).numpy()
    x = rnd(rng.standard_normal((B, 2 * Ho, 2 * Wo, 3)))
    w = rnd(rng.standard_normal((4, 4, 3, Cout)) * 0.1)
    b = rng.standard_normal(Cout).astype(np.float32).astype(np.float64)
    ref = np.maximum(O.conv4s2_fwd(x, w, b), 0)
    rel = lambda a: float(np.linalg.norm(a - ref) / np.linalg.norm(ref))
    good = rel(torch.tensor(ref).to(torch.float32).to(torch.bfloat16).double().numpy())
    trunc = rel(_truncate_bf16(ref).double().numpy())
    tap = rel(torch.tensor(np.maximum(_drop_corner_tap(x, w, b), 0)).to(torch.float32).to(torch.bfloat16).double().numpy())
    print(f"rel-L2 to fp64: rounded {good:.3g}, truncated {trunc:.3g}, one corner tap dropped {tap:.3g} (bound 4e-3)")
    assert good < trunc <= 4e-3 and good < tap <= 4e-3


def test_poisoned_view_and_guards():
    t = torch.arange(2 * 3 * 4 * 5, dtype=torch.float32).reshape(2, 3, 4, 5)
    buf, ptr = E.poisoned_view(t, 16, 8)
    assert buf.shape == (4, 3, 4, 16) and ptr == buf.data_ptr() + (3 * 4 * 16 + 8) * 4
    assert torch.equal(E.view_of(buf, 8, 5), t)
    assert bool(torch.isnan(buf[0]).all()) and bool(torch.isnan(buf[-1]).all())
    assert bool(torch.isnan(buf[..., :8]).all()) and bool(torch.isnan(buf[..., 13:]).all())
    g, p = E.guarded(t)
    assert p == g.data_ptr() + 4 * E.GUARD and torch.equal(E.guarded_data(g, t.shape), t)
    assert bool(torch.isnan(g[:E.GUARD]).all()) and bool(torch.isnan(g[-E.GUARD:]).all())
    out, _ = E.poisoned_view(t, 16, 8, fill=E.SENTINEL)
    before = out.clone()
    inside = (slice(1, -1), Ellipsis, slice(8, 13))
    out[1:-1, ..., 8:13] = 0
    E.assert_outside_untouched(out, before, inside)
    out[0, 0, 0, 0] = 1
    with pytest.raises(AssertionError):
        E.assert_outside_untouched(out, before, inside)
