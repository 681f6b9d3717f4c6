"""gct2_dense_steps_fwd / gct2_dense_steps_bwd (the per-timestep heads of train.py:199, 203, 211-214) per element, on the GPU.

The gathered head is the Dense(3) head with a weight slice picked per image, so its reference is the library's own plain head run image
by image on a contiguous copy of the slice: the forward output and the input gradient must agree with gct2_dense_fwd / gct2_dense_bwd
BIT FOR BIT.  The kernel / bias gradients (written in full, ordered sums, no atomics) are compared with an integer reference formed on
the CPU in float64 on exact-sum inputs (tests/exact_cases.py's practice: small integers in x, small integers times powers of two in dy,
so every partial sum is exact in fp32 in any order).  Every case poisons what must not be read (NaN in the pad channels of x) and guards
what must not be written (sentinels around y, dw, db and the scratch).

Shapes: Cin = 67 / ldx = 72 (the reference head) and Cin = 11 / ldx = 11; steps 1, 5, 200; B = 4; HW = 36 (less than a 128-pixel tile)
and 144 (a tile and a remainder: an image boundary falls inside what would be one tile of the flattened batch);
t_int = [1, steps, 1, min(3, steps)]: both end slices, one slice shared by two images."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F32, BF16, F16 = 0, 1, 2
TD = {F32: torch.float32, BF16: torch.bfloat16, F16: torch.float16}
B = 4
GUARD, SENT = 64, 12345.0
SHAPES = [(67, 72), (11, 11)]
CASES = [pytest.param(dt, cin, ldx, steps, hw, id=f"{'f32 bf16 f16'.split()[dt]}-cin{cin}-steps{steps}-hw{hw}")
         for dt in (F32, BF16, F16) for cin, ldx in SHAPES for steps in (1, 5, 200) for hw in (36, 144)]


def lib():
    import gan_class_transfer2_amd as g
    return g._lib


def stream():
    return torch.cuda.current_stream().cuda_stream


def t_pattern(steps):
    return [1, steps, 1, min(3, steps)]


def guarded(n, gpu, dtype=torch.float32, fill=0.0):
    """(whole buffer, the n elements in the middle): GUARD sentinels on either side"""
    big = torch.full((GUARD + n + GUARD,), SENT, dtype=dtype, device=gpu)
    inner = big[GUARD:GUARD + n]
    inner.fill_(fill)
    return big, inner


def guards_intact(big, n):
    return bool((big[:GUARD] == SENT).all()) and bool((big[GUARD + n:] == SENT).all())


def bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def make_x(gen, dt, hw, cin, ldx, gpu, integers=False):
    if integers:
        v = torch.randint(-3, 4, (B * hw, ldx), generator=gen).float()
    else:
        v = torch.randn(B * hw, ldx, generator=gen)
    v[:, cin:] = float("nan")                                   # pad channels: never read
    return v.to(TD[dt]).to(gpu).contiguous()


def steps_fwd(dt, x, ldx, w, b, t, y, hw, cin, cout, steps, ctx=None):
    lib().call("gct2_dense_steps_fwd", ctx, dt, x.data_ptr(), ldx, w.data_ptr(), b.data_ptr(), t.data_ptr(), y.data_ptr(), B, hw, cin, cout,
               steps, stream())


def scratch_floats(hw, cin, cout):
    need = ctypes.c_size_t(0)
    lib().check(lib().load().gct2_dense_steps_scratch(B, hw, cin, cout, ctypes.byref(need)), "gct2_dense_steps_scratch")
    return need.value


def steps_bwd(dt, x, ldx, w, t, dy, dx, lddx, dw, db, sc, hw, cin, cout, steps, cmask, accumulate):
    lib().call("gct2_dense_steps_bwd", None, dt, x.data_ptr(), ldx, w.data_ptr(), t.data_ptr(), dy.data_ptr(), dx.data_ptr() if dx is not None else None,
               lddx, dw.data_ptr(), db.data_ptr(), sc.data_ptr(), sc.numel(), B, hw, cin, cout, steps, cmask, accumulate, stream())


def slice_copy(w, b, s, cout):
    return w[:, s * cout:(s + 1) * cout].contiguous(), b[s * cout:(s + 1) * cout].contiguous()


@pytest.mark.parametrize("dt, cin, ldx, steps, hw", CASES)
def test_forward_equals_the_plain_head_per_image_bit_for_bit(gpu, dt, cin, ldx, steps, hw):
    gen = torch.Generator().manual_seed(1000 * steps + hw + cin)
    x = make_x(gen, dt, hw, cin, ldx, gpu)
    es = x.element_size()
    for cout in (3, 1, 4):
        w = torch.randn(cin, steps * cout, generator=gen).to(gpu)
        b = torch.randn(steps * cout, generator=gen).to(gpu)
        tl = t_pattern(steps)
        t = torch.tensor(tl, dtype=torch.int32, device=gpu)
        n = B * hw * cout
        big, y = guarded(n, gpu, fill=float("nan"))
        steps_fwd(dt, x, ldx, w, b, t, y, hw, cin, cout, steps)
        ref = torch.full((n,), float("nan"), device=gpu)
        for i, ti in enumerate(tl):
            ws, bs = slice_copy(w, b, ti - 1, cout)
            lib().call("gct2_dense_fwd", dt, x.data_ptr() + i * hw * ldx * es, ldx, ws.data_ptr(), bs.data_ptr(), ref.data_ptr() + 4 * i * hw * cout,
                       hw, cin, cout, stream())
        torch.cuda.synchronize()
        assert bool(torch.isfinite(y).all()) and guards_intact(big, n), (cout,)
        assert torch.equal(bits(y), bits(ref)), (cout, float((y - ref).abs().max()))
        if steps == 1:                                          # one slice: the whole output is ONE plain call
            one = torch.empty(n, device=gpu)
            lib().call("gct2_dense_fwd", dt, x.data_ptr(), ldx, w.data_ptr(), b.data_ptr(), one.data_ptr(), B * hw, cin, cout, stream())
            torch.cuda.synchronize()
            assert torch.equal(bits(y), bits(one))
        # a t_int outside 1..steps is clamped before any address is formed: 0 -> 1, steps + 1 -> steps (the pattern's own slices)
        big2, y2 = guarded(n, gpu, fill=float("nan"))
        t_bad = torch.tensor([0, steps + 1, 1, min(3, steps)], dtype=torch.int32, device=gpu)
        steps_fwd(dt, x, ldx, w, b, t_bad, y2, hw, cin, cout, steps)
        torch.cuda.synchronize()
        assert guards_intact(big2, n) and torch.equal(bits(y2), bits(y)), (cout,)


@pytest.mark.parametrize("dt, cin, ldx, steps, hw", CASES)
def test_backward_dx_equals_the_plain_head_per_image_bit_for_bit(gpu, dt, cin, ldx, steps, hw):
    gen = torch.Generator().manual_seed(2000 * steps + hw + cin)
    cout, cmask = 3, cin - 3
    lddx = cmask + 8                                            # channels [Cmask, lddx) of dx must stay untouched
    x = make_x(gen, dt, hw, cin, ldx, gpu)
    es = x.element_size()
    w = torch.randn(cin, steps * cout, generator=gen).to(gpu)
    dy = torch.randn(B * hw, cout, generator=gen).to(gpu)
    tl = t_pattern(steps)
    t = torch.tensor(tl, dtype=torch.int32, device=gpu)
    dx = torch.full((B * hw, lddx), 7.0, dtype=TD[dt], device=gpu)
    nw, nb = cin * steps * cout, steps * cout
    bigw, dw = guarded(nw, gpu, fill=float("nan"))
    bigb, db = guarded(nb, gpu, fill=float("nan"))
    ns = scratch_floats(hw, cin, cout)
    bigs, sc = guarded(ns, gpu)
    steps_bwd(dt, x, ldx, w, t, dy, dx, lddx, dw, db, sc, hw, cin, cout, steps, cmask, 0)
    ref = torch.full((B * hw, lddx), 7.0, dtype=TD[dt], device=gpu)
    dw_ref, db_ref = torch.zeros(B, cin, cout, device=gpu), torch.zeros(B, cout, device=gpu)
    for i, ti in enumerate(tl):
        ws = w[:, (ti - 1) * cout:ti * cout].contiguous()
        lib().call("gct2_dense_bwd", dt, x.data_ptr() + i * hw * ldx * es, ldx, ws.data_ptr(), dy.data_ptr() + 4 * i * hw * cout,
                   ref.data_ptr() + i * hw * lddx * es, lddx, dw_ref[i].data_ptr(), db_ref[i].data_ptr(), hw, cin, cout, cmask, 0, stream())
    torch.cuda.synchronize()
    assert torch.equal(bits(dx), bits(ref))
    assert bool((dx[:, cmask:].float() == 7.0).all()) and bool(torch.isfinite(dx.float()).all())
    assert guards_intact(bigw, nw) and guards_intact(bigb, nb) and guards_intact(bigs, ns)
    assert bool(torch.isfinite(dw).all()) and bool(torch.isfinite(db).all())
    # the kernel / bias gradients on these random inputs: the plain head's per image (atomics, another order), summed per slice -
    # the fp32 summation bound n 2^-24 sum |x dy| over the n = images x HW terms of an entry
    xf = x[:, :cin].float().double().view(B, hw, cin)
    dyf = (dy.half().float() if dt == F16 else dy).double().view(B, hw, cout)
    dw3, db2 = dw.view(cin, steps, cout).double(), db.view(steps, cout).double()
    for s in sorted(set(v - 1 for v in tl)):
        imgs = [i for i, v in enumerate(tl) if v - 1 == s]
        want = sum(xf[i].T @ dyf[i] for i in imgs)
        bound = len(imgs) * hw * 2.0 ** -24 * sum(xf[i].abs().T @ dyf[i].abs() for i in imgs)
        assert bool(((dw3[:, s] - want).abs() <= bound).all()), s
        wantb = sum(dyf[i].sum(0) for i in imgs)
        assert bool(((db2[s] - wantb).abs() <= len(imgs) * hw * 2.0 ** -24 * sum(dyf[i].abs().sum(0) for i in imgs)).all()), s
    # out-of-range timesteps: clamped (0 -> slice 0, steps + 1 -> slice steps - 1), same outputs, guards intact
    dx2 = torch.full((B * hw, lddx), 7.0, dtype=TD[dt], device=gpu)
    bigw2, dw2 = guarded(nw, gpu, fill=float("nan"))
    bigb2, db2_ = guarded(nb, gpu, fill=float("nan"))
    bigs2, sc2 = guarded(ns, gpu)
    t_bad = torch.tensor([0, steps + 1, 1, min(3, steps)], dtype=torch.int32, device=gpu)
    steps_bwd(dt, x, ldx, w, t_bad, dy, dx2, lddx, dw2, db2_, sc2, hw, cin, cout, steps, cmask, 0)
    torch.cuda.synchronize()
    assert guards_intact(bigw2, nw) and guards_intact(bigb2, nb) and guards_intact(bigs2, ns)
    assert torch.equal(bits(dx2), bits(dx)) and torch.equal(bits(dw2), bits(dw)) and torch.equal(bits(db2_), bits(db))


@pytest.mark.parametrize("dt, cin, ldx, steps, hw", CASES)
def test_backward_dw_db_exact_sums(gpu, dt, cin, ldx, steps, hw):
    """x in {-3..3}, dy = {-3..3} * 2^{-2..2}: every product is a multiple of 1/4 below 48 and an entry sums at most 2 * 144 of them, so
    every partial sum is exact in fp32 in any order, and exact in fp16 / bf16 storage - the result must equal the float64 reference bit
    for bit, slices nobody selected must be +0.0, accumulate must add exactly and two runs must agree in every bit."""
    gen = torch.Generator().manual_seed(3000 * steps + hw + cin)
    cout, cmask = 3, cin - 3
    x = make_x(gen, dt, hw, cin, ldx, gpu, integers=True)
    w = torch.randn(cin, steps * cout, generator=gen).to(gpu)
    dy = (torch.randint(-3, 4, (B * hw, cout), generator=gen).float() * 2.0 ** torch.randint(-2, 3, (B * hw, cout), generator=gen).float()).to(gpu)
    tl = t_pattern(steps)
    t = torch.tensor(tl, dtype=torch.int32, device=gpu)
    nw, nb, ns = cin * steps * cout, steps * cout, scratch_floats(hw, cin, cout)
    # the integer reference, float64 on the CPU
    xf, dyf = x[:, :cin].float().double().cpu().view(B, hw, cin), dy.double().cpu().view(B, hw, cout)
    dw_ref, db_ref = torch.zeros(cin, steps, cout, dtype=torch.float64), torch.zeros(steps, cout, dtype=torch.float64)
    for i, ti in enumerate(tl):
        dw_ref[:, ti - 1] += xf[i].T @ dyf[i]
        db_ref[ti - 1] += dyf[i].sum(0)
    dw_ref, db_ref = (dw_ref + 0.0).float().reshape(-1), (db_ref + 0.0).float().reshape(-1)
    dx = torch.zeros(B * hw, cmask, dtype=TD[dt], device=gpu)
    runs = []
    for _ in range(2):
        bigw, dw = guarded(nw, gpu, fill=float("nan"))
        bigb, db = guarded(nb, gpu, fill=float("nan"))
        bigs, sc = guarded(ns, gpu, fill=float("nan"))
        steps_bwd(dt, x, ldx, w, t, dy, dx, cmask, dw, db, sc, hw, cin, cout, steps, cmask, 0)
        torch.cuda.synchronize()
        assert guards_intact(bigw, nw) and guards_intact(bigb, nb) and guards_intact(bigs, ns)
        runs.append((dw.cpu().clone(), db.cpu().clone()))
    dw, db = runs[0]
    assert torch.equal(bits(dw), bits(dw_ref)) and torch.equal(bits(db), bits(db_ref))
    assert torch.equal(bits(runs[1][0]), bits(dw)) and torch.equal(bits(runs[1][1]), bits(db))
    unused = [s for s in range(steps) if s + 1 not in tl]
    if unused:
        z = dw.view(cin, steps, cout)[:, unused]
        assert bool((bits(z) == 0).all()) and bool((bits(db.view(steps, cout)[unused]) == 0).all())       # +0.0, not -0.0
    # accumulate = 1 on a prefilled dw / db adds exactly
    pre_w = torch.randint(-8, 9, (nw,), generator=gen).float()
    pre_b = torch.randint(-8, 9, (nb,), generator=gen).float()
    bigw, dwa = guarded(nw, gpu)
    bigb, dba = guarded(nb, gpu)
    bigs, sc = guarded(ns, gpu, fill=float("nan"))
    dwa.copy_(pre_w.to(gpu)); dba.copy_(pre_b.to(gpu))
    steps_bwd(dt, x, ldx, w, t, dy, dx, cmask, dwa, dba, sc, hw, cin, cout, steps, cmask, 1)
    torch.cuda.synchronize()
    assert guards_intact(bigw, nw) and guards_intact(bigb, nb) and guards_intact(bigs, ns)
    assert torch.equal(bits(dwa.cpu()), bits(pre_w + dw_ref)) and torch.equal(bits(dba.cpu()), bits(pre_b + db_ref))


def test_launch_log_names_the_calls(gpu):
    c = lib().Context()
    c.log_launches(True)
    gen = torch.Generator().manual_seed(5)
    x = make_x(gen, BF16, 36, 11, 11, gpu)
    w, b = torch.randn(11, 15, generator=gen).to(gpu), torch.zeros(15, device=gpu)
    t = torch.tensor(t_pattern(5), dtype=torch.int32, device=gpu)
    y = torch.empty(B * 36 * 3, device=gpu)
    steps_fwd(BF16, x, 11, w, b, t, y, 36, 11, 3, 5, ctx=c.handle)
    torch.cuda.synchronize()
    assert c.read_launch_log() == ["dense_steps:fwd"]
