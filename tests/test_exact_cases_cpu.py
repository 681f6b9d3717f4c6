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


# ---- the fused head and the fused optimizer step (tests/test_fused_exact_gpu.py) ----------------------------------------------------

def _on_grid(a, step):
    return bool(np.array_equal(np.round(np.asarray(a) / step) * step, a))


def _fp16_normal(a):
    a = np.abs(np.asarray(a))
    a = a[a != 0]
    return bool(((a >= 2.0 ** -14) & (a < 65504)).all())


# 16-bit stores at which the 5 % / 0.5 % shares are out of reach under the budget, so only "some inexact, some ties" is asserted:
#   head_train, fp16, M = 32775: db_dx sums |dx| over 32775 pixels (half of them masked), so the MEAN |dx| stays below
#     2^22 / 16387 = 256 steps, and fp16 holds every integer up to 2048: at most 256 / 2048 = 12.5 % of the elements could reach
#     the rounding range even if all the mass sat there, a realistic spread gets well under 5 %;
#   convT_head, fp16: the same with head_dw = y^T dpred: y of about 1500 steps (so that its own conversion rounds) over 1024 / 4096
#     pixels leaves a mean |delta| near 1, |dy| = |delta . w| near 100 steps.
# A few pixels with a large residual (exact_cases' tails) take those stores into the rounding range.
FEW_ROUNDINGS_AT_DX = {("head_train", (32775, 67, 3), F16), ("convT_head", (1, 16, 16, 8), F16), ("convT_head", (2, 16, 32, 136), F16)}


@pytest.mark.parametrize("case", [c for c in E.fused_cases() if c[3] is None], ids=_id)
def test_fused_head_inputs(case):
    """conditions on the inputs of the exact head cases, met by the reference alone: storage types, the budget of every reduction on
    the arrays as drawn, exactness of every reference in float32, both mask values, rounding and ties at the 16-bit stores, no fp16
    overflow or subnormal, and a loss scale that makes the gradient scale a power of two"""
    c = E.make_case(*case)
    M = c.x.shape[0]
    assert E.survives_storage(c.x, c.dt) and E.survives_storage(c.w, F32) and E.survives_storage(c.bias, F32) and E.survives_storage(c.target, F32)
    for name, total, step in E.head_budgets(c, c.x):
        assert total / step < E.BUDGET, (name, total / step)
    for a, step in ((c.x, c.x_step), (c.w, 2.0 ** -c.sw), (c.bias, c.lsb), (c.pred, c.lsb), (c.target, c.lsb), (c.dpred, c.dp_step),
                    (c.dx, c.dx_step), (c.prev_dw, c.x_step * c.dp_step), (c.prev_db, c.dp_step), (c.prev_db_dx, c.dx_step)):
        assert _on_grid(a, step)
    assert np.array_equal(c.d, c.delta * c.lsb) and float((c.delta ** 2).sum()) < 2.0 ** 24
    for r in (c.pred, c.pred_r, c.d, c.dpred, c.dx, c.dw, c.db, c.db_dx, c.db_dx_stored, c.dw + c.prev_dw, c.db + c.prev_db,
              c.db_dx + c.prev_db_dx, c.db_dx_stored + c.prev_db_dx):
        E.expected(r, F32)
    # the gradient scale as the kernels form it: fl(fl(scale * 2) / fl(M * Cout)), a power of two
    n = np.float32(M) * np.float32(3)
    assert float(np.float32(c.loss_scale)) == c.loss_scale and float(n) == 3.0 * M
    assert float(np.float32(np.float32(c.loss_scale) * np.float32(2)) / n) == c.gscale == 2.0 ** (c.j + 1) and c.j >= 0
    # the two-term operands of the matrix-core backward pass: weights within 16 bits, and never a low term in both factors
    s = E.SIG_BITS[c.dt]
    low = lambda a: E._round_to(a, c.dt) != a
    assert _on_grid(c.w * 2.0 ** c.sw, 1.0) and np.abs(c.w).max() * 2.0 ** c.sw < (1 << 2 * s)
    assert not (low(c.w[:64]).any(0) & low(c.dpred).any(0)).any()
    if c.dt == BF16 and 16 <= M <= 4096:        # (at M = 32775 the budget leaves dpred 4 bits: no low term there; fp16 holds dpred in one)
        assert low(c.w[:64, 0]).any() and low(c.dpred[:, 1]).any(), "no operand needs its low term"
    mask = c.x[:, :64] > 0
    assert 0.1 <= float(mask.mean()) <= 0.9
    key = (c.entry, c.shape, c.dt)
    stores = [(c.g, c.dt, key not in FEW_ROUNDINGS_AT_DX)] + ([(c.pred, F16, True)] if c.dt == F16 else [])
    for ref, dt, rounds in stores:
        inexact, ties = rounding_shares(ref, dt)
        if rounds and M >= 1000:
            assert inexact >= MIN_INEXACT and ties >= MIN_TIES, (inexact, ties)
        else:                            # 5 and 16 pixels: at least one of each kind; FEW_ROUNDINGS_AT_DX: a hundred
            need = 1 if rounds else 100
            assert inexact * ref.size >= need and ties * ref.size >= need, (inexact, ties)
    if c.dt == F16:
        for a in (c.x, c.pred_r, c.dpred, c.dx, c.target):
            assert _fp16_normal(a)
    if c.entry == "convT_head":
        E.assert_budget(c.ops)
        assert E.survives_storage(c.xc, c.dt) and E.survives_storage(c.wc, c.dt) and E.survives_storage(c.bc, F32)
        E.expected(c.y, F32)
        pos = c.y > 0
        assert float((c.yr != c.y)[pos].mean()) >= 0.05 and np.abs(c.y).max() < 65504
        inexact, ties = rounding_shares(c.y[pos], c.dt)
        assert ties >= MIN_TIES, ties


@pytest.mark.parametrize("case", [c for c in E.fused_cases() if c[3] == "wide"], ids=_id)
def test_wide_head_inputs(case):
    """the one inexact head case: weights with 24 significant bits, a residual that needs more than one term of the storage type"""
    c = E.make_case(*case)
    assert E.survives_storage(c.x, c.dt) and E.survives_storage(c.w, F32) and E.survives_storage(c.target, F32)
    bits = np.round(np.abs(c.w) * 2.0 ** 24).astype(np.int64)
    assert float(np.mean((bits >= 1 << 23) & (bits & 1 == 1))) >= 0.2          # all 24 bits in use
    d = c.pred - c.target
    assert np.abs(c.delta).max() > 1 << 11 and float(np.mean(E._round_to(d, c.dt) != d)) >= 0.5
    dp = d * c.gscale
    assert _fp16_normal(dp) and np.abs(c.pred).max() < 65504
    assert 0.1 <= float((c.x[:, :64] > 0).mean()) <= 0.9


@pytest.mark.parametrize("case", E.adam_cases(), ids=_id)
def test_fused_adam_gradient_inputs(case):
    """the weight-gradient cases of the fused optimizer step: the usual budget - the gradient is then the same fp32 tensor whatever
    the number of slabs - and a gradient that is not trivially zero"""
    c = E.make_case(*case)
    E.assert_budget(c.ops)
    assert E.survives_storage(c.ops.a, c.dt) and E.survives_storage(c.ops.b, c.dt)
    g = E.expected(c.dw, F32)
    E.expected(c.db, F32)
    assert float((g != 0).float().mean()) >= 0.9 and c.dw.size % 4 == 0
