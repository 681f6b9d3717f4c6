"""Progressive distillation on the host: the teacher's grid and its table (trainer_math.distill_grid / distill_table) against doubles,
and the arithmetic of gct2_distill_target as tests/distill_cases.py restates it - the property that defines the target, in float64 and
within a rounding bound in float32."""
import numpy as np
import pytest

import distill_cases as D
from oracle import denoiser_oracle as O


def tm():
    import gan_class_transfer2_amd as g
    return g.trainer_math


GRIDS = [(200, 100), (200, 25), (200, 1), (6, 3), (6, 1)]


@pytest.mark.parametrize("steps,n", GRIDS)
def test_grid_identity(steps, n):
    """the student's grid is the odd half of the teacher's: a distilled student is sampled with plain generate(num_steps=N)"""
    T = tm()
    taus = T.distill_grid(steps, n)
    assert len(taus) == 2 * n and taus == T.sampling_timesteps(steps, 2 * n) and taus[-1] == steps
    assert taus[1::2] == T.sampling_timesteps(steps, n)
    assert all(b > a for a, b in zip(taus, taus[1:])) and taus[0] >= 1
    assert T.distill_grid(steps, n, timesteps=taus) == taus
    assert T.DISTILL_STREAM_PAIR == 8 and T.DISTILL_STREAM_EPS == 9


def test_grid_refusals():
    T = tm()
    for steps, n in ((200, 0), (200, 101), (6, 4), (200, -1), (200, 2.0), (200, True)):
        with pytest.raises(ValueError):
            T.distill_grid(steps, n)
    for given in ([1, 2, 3], [1, 2, 2, 4], [0, 1, 2, 3], [1, 2, 3, 201], [4, 3, 2, 1], [1, 2, 3, 4.0], [1, 2, 3, 4, 5, 6]):
        with pytest.raises(ValueError):
            T.distill_grid(200, 2, timesteps=given)
    assert T.distill_grid(200, 2, timesteps=[3, 50, 120, 200]) == [3, 50, 120, 200]


@pytest.mark.parametrize("schedule", [None, "cosine"])
@pytest.mark.parametrize("steps,n", GRIDS)
def test_table_against_doubles(steps, n, schedule):
    T = tm()
    taus = T.distill_grid(steps, n)
    alpha = (lambda t: float(O.alpha_dash(t, steps))) if schedule is None else (lambda t: float(T.alpha_dash(t, steps, schedule, 0.0)))
    alphas = D.pair_alphas(taus, alpha)
    tab, tt = T.distill_table(taus, steps, schedule, 0.0)
    assert tab.dtype == np.float32 and tab.shape == (n, D.ROW) and tt.dtype == np.int32 and tt.shape == (n, 2)
    want = D.table_f32(alphas)
    assert np.array_equal(tab.view(np.int32), want.view(np.int32))
    assert tt.tolist() == [[taus[2 * j - 1], taus[2 * j - 2]] for j in range(1, n + 1)]
    # the end point of pair 1 is alpha = 1: the x0 estimate itself
    assert tab[0, D.SA2:D.DEN + 1].tolist() == [1.0, 0.0, 0.0, 1.0]
    # every root is the double root rounded once; r and den come from the double roots, not from the rounded ones
    t64 = D.table_f64(alphas)
    assert np.array_equal(tab[:, :8], t64.astype(np.float32))
    assert (t64[:, D.DEN] > t64[:, D.SA2] - t64[:, D.SA0]).all() or n == 1
    assert (tab[:, D.DEN] > 0).all() and (tab[:, D.SB0] > 0).all()
    # generate's float32 roots of float32 alphas against the double roots: sqrtf((float)a) halves the relative error of the cast and
    # stays within one unit in the last place; 1.f - (float)a carries an ABSOLUTE error of up to 2^-24, which the root turns into
    # 2^-24 / (2 sb) - many units in the last place where alpha is close to 1 (the low timesteps of "cosine").  That is why the table
    # holds both pairs: the sibling kernels' bits need the float32 forms
    for a, b in ((D.CX0, D.SA0), (D.CX1, D.SA1)):
        assert (np.abs(tab[:, a].astype(np.float64) - tab[:, b]) <= np.spacing(tab[:, b])).all()
    for a, b in ((D.CK0, D.SB0), (D.CE1, D.SB1)):
        assert (np.abs(tab[:, a].astype(np.float64) - tab[:, b]) <= 2.0 ** -24 / tab[:, b] + np.spacing(tab[:, b])).all()


def test_table_refusals():
    T = tm()
    with pytest.raises(ValueError):                      # an odd number of timesteps, a grid that does not increase
        T.distill_table([1, 2, 3], 200)
    with pytest.raises(ValueError):
        T.distill_table([1, 3, 2, 4], 200)
    rising = lambda t01: 0.1 + 0.5 * t01                 # alpha grows with t: den < 0
    with pytest.raises(ValueError, match="den"):
        T.distill_table([2, 4, 6, 8], 8, rising, 0.0)
    flat = lambda t01: 0.5 + 0.0 * t01                   # alpha constant: den = 0
    with pytest.raises(ValueError, match="den"):
        T.distill_table([2, 4, 6, 8], 8, flat, 0.0)
    zero = lambda t01: max(0.0, 0.9 - 1.2 * t01)         # alpha = 0 at the last timesteps: legal for X and V, refused for the epsilon modes
    taus = [1, 2, 7, 8]
    T.distill_table(taus, 8, zero, 0.0, mode=D.SAMPLE_X)
    T.distill_table(taus, 8, zero, 0.0, mode=D.SAMPLE_V)
    for mode in (D.SAMPLE_EPS, D.SAMPLE_SCALED_EPS):
        with pytest.raises(ValueError, match="divides"):
            T.distill_table(taus, 8, zero, 0.0, mode=mode)
    with pytest.raises(ValueError):                      # alpha = 1 at a timestep the teacher evaluates
        T.distill_table([1, 2], 8, lambda t01: 1.0, 0.0)


def _tables(steps=D.STEPS, n=D.N):
    T = tm()
    taus = T.distill_grid(steps, n)
    alphas = D.pair_alphas(taus, lambda t: float(O.alpha_dash(t, steps)))
    return D.table_f64(alphas), D.table_f32(alphas)


PAIR_SETS = [np.arange(1, D.N + 1), np.array(D.PAIRS)]


@pytest.mark.parametrize("mode", D.MODES, ids=D.MODE_IDS)
def test_defining_property_in_float64(mode):
    """one DDIM step from z0 with the estimate x~ to alpha'' equals the z'' of the teacher's two steps, for arbitrary predictions, at
    every pair of the grid: 1e-12 relative"""
    t64, _ = _tables()
    pair = PAIR_SETS[0]
    r = D.rows_of(t64, pair)
    rng = np.random.default_rng([mode, 5])
    p1, p2, z0 = (rng.standard_normal((len(pair), 64)) for _ in range(3))
    _, x2, e2 = D.two_steps_f64(mode, r, p1, p2, z0)
    xt, et, z2 = D.solve_f64(r, x2, e2, z0)
    one_step = r[:, D.SA2] * xt + r[:, D.SB2] * et           # the student's step: its estimate xt, eps re-derived from z0
    err = np.abs(one_step - z2).max() / np.abs(z2).max()
    print(f"defining property, mode {mode}: relative error {err:.3g}")
    assert err <= 1e-12
    # and the student's input: sa0 xt + sb0 et is z0
    assert np.abs(r[:, D.SA0] * xt + r[:, D.SB0] * et - z0).max() <= 1e-12 * np.abs(z0).max()


@pytest.mark.parametrize("mode", D.MODES, ids=D.MODE_IDS)
def test_perfect_teacher_in_float64(mode):
    """predictions built so that the teacher's estimates are the clean image and the noise at both steps: x~ = x and eps~ = eps"""
    t64, _ = _tables()
    pair = PAIR_SETS[0]
    r = D.rows_of(t64, pair)
    rng = np.random.default_rng([mode, 6])
    x, e = (rng.standard_normal((len(pair), 64)) for _ in range(2))
    z0 = r[:, D.SA0] * x + r[:, D.SB0] * e
    p1 = D.prediction_f64(mode, x, e, r[:, D.SA0], r[:, D.SB0])
    p2 = D.prediction_f64(mode, x, e, r[:, D.SA1], r[:, D.SB1])
    z1, x2, e2 = D.two_steps_f64(mode, r, p1, p2, z0)
    assert np.abs(z1 - (r[:, D.SA1] * x + r[:, D.SB1] * e)).max() <= 1e-12
    xt, et, _ = D.solve_f64(r, x2, e2, z0)
    print(f"perfect teacher, mode {mode}: |xt - x| {np.abs(xt - x).max():.3g}, |et - eps| {np.abs(et - e).max():.3g}")
    # (x is recovered through divisions by sqrt(alpha) >= 0.0025 in the epsilon modes, eps through 1 / den <= 1 / (sa2 - sa0))
    assert np.abs(xt - x).max() <= 1e-9 and np.abs(et - e).max() <= 1e-9


@pytest.mark.parametrize("mode", D.MODES, ids=D.MODE_IDS)
@pytest.mark.parametrize("which", range(len(PAIR_SETS)), ids=["every_pair", "kernel_pairs"])
def test_defining_property_in_float32(mode, which):
    """the float32 restatement against the float64 solve fed the SAME float32 x2, e2, z0: six roundings in the expression and the two
    table roundings (r, den; sa2, sb2 enter a product each) bound the elementwise error of xt by
    8 x 2^-24 (|sa2 x2| + |sb2 e2| + |r z0|) / den"""
    t64, t32 = _tables()
    pair = PAIR_SETS[which]
    rng = np.random.default_rng([mode, which, 7])
    p2, z1, z0 = (rng.standard_normal((len(pair), 1024)).astype(np.float32) for _ in range(3))
    xt, et, x2, e2 = D.target_f32(mode, t32, pair, p2, z1, z0, 0.0)
    r = D.rows_of(t64, pair)
    want, _, _ = D.solve_f64(r, x2, e2, z0)
    bound = 8 * 2.0 ** -24 * (np.abs(r[:, D.SA2] * x2) + np.abs(r[:, D.SB2] * e2.astype(np.float64)) + np.abs(r[:, D.RR] * z0)) / r[:, D.DEN]
    err = np.abs(xt.astype(np.float64) - want)
    live = bound > 0
    ratio = float((err[live] / bound[live]).max())
    print(f"float32 target, mode {mode}, {['every pair', 'kernel pairs'][which]}: worst error / bound {ratio:.3f}")
    assert (err <= bound).all(), ratio


@pytest.mark.parametrize("mode", D.MODES, ids=D.MODE_IDS)
def test_pair_one_returns_the_estimate(mode):
    """pair 1 has no t'': xt is x2's bits (a select, so an infinite or NaN eps never reaches it), with and without the clip"""
    _, t32 = _tables()
    pair = np.ones(D.B, dtype=np.int64)
    p2, z1, z0, _ = D.planes(D.B, D.NPIXS[0] * D.C)
    for clip in D.CLIPS:
        xt, _, x2, _ = D.target_f32(mode, t32, pair, p2, z1, z0, clip)
        same = (xt.view(np.int32) == x2.view(np.int32)) | (np.isnan(xt) & np.isnan(x2))
        assert same.all()
        if clip:
            assert np.nanmax(np.abs(xt)) <= clip
    # pair values outside 1..N act as 1 and N
    a = D.target_f32(mode, t32, np.array([0, D.N + 5, -7]), p2, z1, z0, 0.0)
    b = D.target_f32(mode, t32, np.array([1, D.N, 1]), p2, z1, z0, 0.0)
    assert all(np.array_equal(u.view(np.int32), v.view(np.int32)) for u, v in zip(a, b))


@pytest.mark.parametrize("mode", D.MODES, ids=D.MODE_IDS)
def test_student_input_lands_on_z0(mode):
    """fl(fl(sa0 xt) + fl(sb0 et)) against z0.  With A = fl(sa0 xt): et = (z0 - A) / sb0 carries two roundings, sb0 et a third, the sum a
    fourth, so |result - z0| <= 2^-24 (3 |z0 - A| + |z0|) to first order - a few units in the last place of z0 where sa0 xt and z0 are of
    one size, more where they cancel.  This is what the student's input differs from the teacher's z_t by"""
    _, t32 = _tables()
    pair = PAIR_SETS[0]
    rng = np.random.default_rng([mode, 8])
    p2, z1, z0 = (rng.standard_normal((len(pair), 1024)).astype(np.float32) for _ in range(3))
    xt, et, _, _ = D.target_f32(mode, t32, pair, p2, z1, z0, 1.0)
    back = D.student_input_f32(t32, pair, xt, et)
    r = D.rows_of(t32, pair)
    A = (r[:, D.SA0] * xt).astype(np.float64)
    bound = 2.0 ** -24 * (3 * np.abs(z0 - A) + np.abs(z0)) * 1.001
    err = np.abs(back.astype(np.float64) - z0)
    ulps = float((err / np.spacing(np.abs(z0))).max())
    print(f"student input, mode {mode}: worst distance {ulps:.1f} ulps of z0, worst error / bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all()


def test_symbols_and_version():
    import gan_class_transfer2_amd as g
    L = g._lib
    for name in ("gct2_distill_start", "gct2_distill_step", "gct2_distill_target"):
        assert name in L.SIGNATURES and name in L.PLANNABLE and hasattr(L.load(), name)
    assert L.load().gct2_abi_version() == 17 == L.ABI_VERSION
    assert L.DISTILL_ROW == D.ROW == len(g.trainer_math.DISTILL_COLUMNS)
    assert callable(g.Distiller) and callable(g.clone_denoiser) and callable(g.progressive_distill)
