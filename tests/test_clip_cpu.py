"""CPU tier of gradient clipping (Keras Adam(clipnorm / global_clipnorm / clipvalue) [TF]): the three C functions are declared,
exported and bound, the two launching ones plannable; the host-only layout and every rejection of the launching calls need no device;
the optimizer translation and the engines' call lists; and the numpy restatement (tests/clip_cases.py) on its own corner cases."""
import ctypes
import types

import numpy as np
import pytest

import clip_cases as K
import gan_class_transfer2_amd as g

P = 4096                    # a fake, 16-byte aligned device address: every launching call below is rejected before anything reads it
EINVAL = 1
NONE, VALUE, NORM, GLOBAL = K.CLIP_NONE, K.CLIP_VALUE, K.CLIP_NORM, K.CLIP_GLOBAL_NORM


class Seg(ctypes.Structure):
    """gct2_sumsq_seg"""
    _fields_ = [("begin", ctypes.c_uint64), ("count", ctypes.c_uint64), ("first_partial", ctypes.c_uint64)]


def run_layout(begin, count, nseg=None, fill=7):
    lib = g._lib.load()
    n = len(begin)
    b, c = (ctypes.c_uint64 * max(n, 1))(*begin), (ctypes.c_uint64 * max(n, 1))(*count)
    out = (Seg * max(n, 1))()
    for s in out:
        s.begin = s.count = s.first_partial = fill
    npart = ctypes.c_size_t(fill)
    rc = lib.gct2_sumsq_layout(b, c, n if nseg is None else nseg, out, ctypes.byref(npart))
    return rc, [(s.begin, s.count, s.first_partial) for s in out][:n], npart.value, lib.gct2_last_error().decode()


# ---- declared, exported, bound, plannable ------------------------------------------------------------------------------------------
def test_the_three_functions_are_exported_bound_and_the_launching_ones_plannable():
    L = g._lib
    lib = L.load()
    raw = ctypes.CDLL(L.LIB_PATH)
    vp, i, f, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t
    assert all(hasattr(raw, n) for n in ("gct2_sumsq_layout", "gct2_grad_sumsq", "gct2_adam_keras_clipped"))
    assert L.SIGNATURES["gct2_sumsq_layout"] == [vp, vp, i, vp, ctypes.POINTER(ctypes.c_size_t)]
    assert L.SIGNATURES["gct2_grad_sumsq"] == [vp, vp, i, sz, f, vp, vp, vp, vp]
    assert L.SIGNATURES["gct2_adam_keras_clipped"] == [vp, vp, vp, vp, vp, i, sz, f, f, f, f, f, vp, i, f, vp, vp]
    assert {"gct2_grad_sumsq", "gct2_adam_keras_clipped"} <= L.PLANNABLE and "gct2_sumsq_layout" not in L.PLANNABLE
    assert lib.gct2_abi_version() == L.ABI_VERSION == 17              # additions change no signature
    assert (L.CLIP_NONE, L.CLIP_VALUE, L.CLIP_NORM, L.CLIP_GLOBAL_NORM) == (NONE, VALUE, NORM, GLOBAL) == (0, 1, 2, 3)
    assert (L.SUMSQ_CHUNK, L.SUMSQ_MAX_SEGMENTS) == (K.CHUNK, K.MAX_SEGMENTS) and K.CHUNK % 4 == 0 and K.MAX_SEGMENTS >= 256
    header = open(g._lib.os.path.join(g._lib._HERE, "..", "include", "gct2.h")).read()
    assert f"#define GCT2_SUMSQ_CHUNK {K.CHUNK}" in header and f"#define GCT2_SUMSQ_MAX_SEGMENTS {K.MAX_SEGMENTS}" in header
    for name, nargs, text in (("gct2_grad_sumsq", 9, b"grad_sumsq: null pointer"), ("gct2_adam_keras_clipped", 17, b"adam_keras_clipped: null pointer")):
        plan = L.Plan()
        idx = ctypes.c_int(-1)
        arr = (ctypes.c_uint64 * nargs)()
        assert lib.gct2_plan_add_call(plan.handle, name.encode(), arr, nargs, ctypes.byref(idx)) == 0 and idx.value == 0
        assert lib.gct2_plan_add_call(plan.handle, name.encode(), arr, nargs - 1, None) == EINVAL
        assert b"takes %d arguments" % nargs in lib.gct2_last_error()
        # the recorded call (all-zero arguments) is rejected by its own checks when the plan runs: nothing is launched
        failed = ctypes.c_int(-1)
        assert lib.gct2_plan_run(plan.handle, 0, 1, ctypes.byref(failed)) == EINVAL and failed.value == 0
        assert text in lib.gct2_last_error()
    plan = L.Plan()
    assert lib.gct2_plan_add_call(plan.handle, b"gct2_sumsq_layout", (ctypes.c_uint64 * 5)(), 5, None) == EINVAL
    assert b"not an entry point a plan can hold" in lib.gct2_last_error()


# ---- gct2_sumsq_layout ---------------------------------------------------------------------------------------------------------------
def test_layout_prefix_and_partial_counts():
    C = K.CHUNK
    lengths = (1, C - 1, C, C + 1, 3 * C + 7, 2 * C)
    segs, _ = K.layout(lengths)
    rc, out, npart, _ = run_layout([b for b, _ in segs], [c for _, c in segs])
    assert rc == 0
    counts = [1, 1, 1, 2, 4, 2]
    assert K.partial_counts(segs) == counts
    assert out == [(b, c, sum(counts[:s])) for s, (b, c) in enumerate(segs)] and npart == sum(counts) == 11
    for n, want in ((1, 1), (C - 1, 1), (C, 1), (C + 1, 2)):                    # alone, at begin 0
        assert run_layout([0], [n])[1:3] == ([(0, n, 0)], want)
    # adjacent segments (no padding between them) are fine; the table's maximum length is accepted
    assert run_layout([0, 4, 8], [4, 4, 1])[0] == 0
    rc, out, npart, _ = run_layout([4 * s for s in range(K.MAX_SEGMENTS)], [3] * K.MAX_SEGMENTS)
    assert rc == 0 and npart == K.MAX_SEGMENTS and out[-1] == (4 * (K.MAX_SEGMENTS - 1), 3, K.MAX_SEGMENTS - 1)


@pytest.mark.parametrize("begin, count, nseg, text", [
    ([64, 0], [4, 4], None, "ascending order"),                    # unsorted
    ([0, 64, 32], [4, 4, 4], None, "ascending order"),
    ([0, 4], [5, 4], None, "overlap"),                             # overlapping
    ([0, 0], [4, 4], None, "overlap"),
    ([0, 66], [4, 4], None, "not a multiple of 4"),                # begin % 4 != 0
    ([2], [4], None, "not a multiple of 4"),
    ([0, 64], [4, 0], None, "is empty"),                           # zero count
    ([0], [4], 0, "outside [1, 1024]"),                            # nseg 0, negative, above the maximum
    ([0], [4], -1, "outside [1, 1024]"),
    ([0], [4], K.MAX_SEGMENTS + 1, "outside [1, 1024]"),
])
def test_layout_rejects_and_fills_nothing(begin, count, nseg, text):
    rc, out, npart, msg = run_layout(begin, count, nseg)
    assert rc == EINVAL and msg.startswith("sumsq_layout: ") and text in msg, msg
    assert all(s == (7, 7, 7) for s in out) and npart == 7         # validated before anything is filled


def test_layout_rejects_null_pointers():
    lib = g._lib.load()
    b, out, n = (ctypes.c_uint64 * 1)(0), (Seg * 1)(), ctypes.c_size_t(0)
    c = (ctypes.c_uint64 * 1)(4)
    for args in ((None, c, 1, out, ctypes.byref(n)), (b, None, 1, out, ctypes.byref(n)), (b, c, 1, None, ctypes.byref(n)), (b, c, 1, out, None)):
        assert lib.gct2_sumsq_layout(*args) == EINVAL and lib.gct2_last_error() == b"sumsq_layout: null pointer"


# ---- the launching calls reject before any launch --------------------------------------------------------------------------------
def _sumsq(**o):
    a = dict(g=P, segs=P + 4096, nseg=3, npartials=5, grad_mul=1.0, ls=None, partials=P + 8192, sumsq=P + 12288, stream=None)
    assert not set(o) - set(a)
    a.update(o)
    return list(a.values())


@pytest.mark.parametrize("args, text", [
    (_sumsq(g=None), "null pointer"),
    (_sumsq(segs=None), "null pointer"),
    (_sumsq(partials=None), "null pointer"),
    (_sumsq(sumsq=None), "null pointer"),
    (_sumsq(nseg=0), "nseg = 0 outside [1, 1024]"),
    (_sumsq(nseg=-2), "nseg = -2 outside [1, 1024]"),
    (_sumsq(nseg=K.MAX_SEGMENTS + 1, npartials=5000), "outside [1, 1024]"),
    (_sumsq(npartials=0), "npartials = 0"),
    (_sumsq(npartials=2), "npartials = 2 is not what gct2_sumsq_layout reports for 3 segments"),
    (_sumsq(g=P + 8), "g must be 16-byte aligned"),
    (_sumsq(g=P + 4), "g must be 16-byte aligned"),
    (_sumsq(segs=P + 4096 + 4), "8-byte aligned"),
    (_sumsq(partials=P + 8192 + 4), "8-byte aligned"),
    (_sumsq(sumsq=P + 12288 + 4), "8-byte aligned"),
])
def test_grad_sumsq_rejects_bad_arguments_without_a_device(args, text):
    lib = g._lib.load()
    assert lib.gct2_grad_sumsq(*args) == EINVAL
    msg = lib.gct2_last_error().decode()
    assert msg.startswith("grad_sumsq: ") and text in msg, msg


def _adam(**o):
    a = dict(p=P, m=P + 4096, v=P + 8192, g=P + 12288, shadow=None, dtype=g.F32, n=1024, alpha=1e-3, beta1=0.9, beta2=0.999, eps=1e-7,
             grad_mul=1.0, ls=None, mode=NONE, clip=0.0, sumsq=None, stream=None)
    assert not set(o) - set(a)
    a.update(o)
    return list(a.values())


S = P + 65536               # a fake, 8-byte aligned address for sumsq


@pytest.mark.parametrize("args, text", [
    (_adam(p=None), "null pointer"),
    (_adam(m=None), "null pointer"),
    (_adam(v=None), "null pointer"),
    (_adam(g=None), "null pointer"),
    (_adam(n=0), "n == 0"),
    (_adam(p=P + 8), "16-byte aligned"),
    (_adam(m=P + 4096 + 4), "16-byte aligned"),
    (_adam(v=P + 8192 + 8), "16-byte aligned"),
    (_adam(g=P + 12288 + 4), "16-byte aligned"),
    (_adam(shadow=P + 16384 + 4, dtype=g.BF16), "8-byte aligned"),
    (_adam(mode=GLOBAL, clip=1.0, sumsq=S + 4), "8-byte aligned"),
    (_adam(shadow=P + 16384, dtype=g.F32), "16-bit dtype"),
    (_adam(shadow=P + 16384, dtype=7), "16-bit dtype"),
    (_adam(mode=4, clip=1.0), "unknown clip_mode 4"),
    (_adam(mode=-1, clip=1.0), "unknown clip_mode -1"),
    (_adam(mode=VALUE, clip=0.0), "must be finite and > 0"),
    (_adam(mode=VALUE, clip=-1.0), "must be finite and > 0"),
    (_adam(mode=NORM, clip=float("inf"), sumsq=S), "must be finite and > 0"),
    (_adam(mode=GLOBAL, clip=float("nan"), sumsq=S), "must be finite and > 0"),
    (_adam(mode=NORM, clip=1.0), "clip_mode 2 needs sumsq"),
    (_adam(mode=GLOBAL, clip=1.0), "clip_mode 3 needs sumsq"),
])
def test_adam_keras_clipped_rejects_bad_arguments_without_a_device(args, text):
    lib = g._lib.load()
    assert lib.gct2_adam_keras_clipped(*args) == EINVAL
    msg = lib.gct2_last_error().decode()
    assert msg.startswith("adam_keras_clipped: ") and text in msg, msg


def _update(entry, **o):
    """the argument list of one of the three update entry points (RMSprop with momentum where the caller chooses the kind: both slots
    in use, like Adam), valid except for what `o` replaces"""
    a = dict(p=P, g=P + 12288, shadow=None, dtype=g.BF16, n=1024, mode=NONE, clip=0.0, sumsq=None)
    assert not set(o) - set(a)
    a.update(o)
    arenas = [a["p"], P + 4096, P + 8192, a["g"], a["shadow"], a["dtype"], a["n"]]
    clipping = [1.0, None, a["mode"], a["clip"], a["sumsq"]]
    if entry == "gct2_adam_keras_clipped":
        return arenas + [1e-3, 0.9, 0.999, 1e-7] + clipping + [None]
    args = [2] + arenas + [1e-3, 0.9, 0, 0.9, 1e-7] + clipping
    return args + ([1e-6, 0, None] if entry == "gct2_optimizer_apply_reg" else [None])


UPDATE_ENTRIES = ("gct2_adam_keras_clipped", "gct2_optimizer_apply", "gct2_optimizer_apply_reg")
# one bad argument of each class and the full message of each entry point, in UPDATE_ENTRIES' order
UPDATE_REJECTIONS = {
    "null_p": (dict(p=None), ("adam_keras_clipped: null pointer", "optimizer_apply: null pointer", "optimizer_apply_reg: null pointer")),
    "n_zero": (dict(n=0), ("adam_keras_clipped: n == 0", "optimizer_apply: n == 0", "optimizer_apply_reg: n == 0")),
    "misaligned_g": (dict(g=P + 12288 + 4),
                     ("adam_keras_clipped: p, m, v and g must be 16-byte aligned, the shadow and sumsq 8-byte aligned",
                      "optimizer_apply: p, g and the slots in use must be 16-byte aligned, the shadow and sumsq 8-byte aligned",
                      "optimizer_apply_reg: p, g and the slots in use must be 16-byte aligned, the shadow and sumsq 8-byte aligned")),
    "shadow_dtype": (dict(shadow=P + 16384, dtype=7),
                     ("adam_keras_clipped: a shadow needs a 16-bit dtype (GCT2_BF16 / GCT2_F16), got 7",
                      "optimizer_apply: a shadow needs a 16-bit dtype (GCT2_BF16 / GCT2_F16), got 7",
                      "optimizer_apply_reg: a shadow needs a 16-bit dtype (GCT2_BF16 / GCT2_F16), got 7")),
    "clip_mode": (dict(mode=4, clip=1.0),
                  ("adam_keras_clipped: unknown clip_mode 4", "optimizer_apply: unknown clip_mode 4", "optimizer_apply_reg: unknown clip_mode 4")),
    "clip_not_finite": (dict(mode=VALUE, clip=float("inf")),
                        ("adam_keras_clipped: clip = inf must be finite and > 0", "optimizer_apply: clip = inf must be finite and > 0",
                         "optimizer_apply_reg: clip = inf must be finite and > 0")),
    "norm_without_sumsq": (dict(mode=NORM, clip=1.0),
                           ("adam_keras_clipped: clip_mode 2 needs sumsq (gct2_grad_sumsq)", "optimizer_apply: clip_mode 2 needs sumsq (gct2_grad_sumsq)",
                            "optimizer_apply_reg: clip_mode 2 needs sumsq (gct2_grad_sumsq / gct2_grad_sumsq_l2)")),
}


@pytest.mark.parametrize("entry", UPDATE_ENTRIES)
@pytest.mark.parametrize("bad", UPDATE_REJECTIONS)
def test_the_three_update_entry_points_reject_alike_without_a_device(bad, entry):
    """the same bad argument to all three: GCT2_EINVAL before any launch, and the whole message of that entry point"""
    lib = g._lib.load()
    change, messages = UPDATE_REJECTIONS[bad]
    assert getattr(lib, entry)(*_update(entry, **change)) == EINVAL
    assert lib.gct2_last_error().decode() == messages[UPDATE_ENTRIES.index(entry)]


# ---- the public surface ------------------------------------------------------------------------------------------------------------
def test_adam_validates_the_clipping_arguments():
    for kw in (dict(clipnorm=1.0, clipvalue=0.5), dict(clipnorm=1.0, global_clipnorm=1.0), dict(global_clipnorm=2.0, clipvalue=0.5),
               dict(clipnorm=1.0, global_clipnorm=1.0, clipvalue=1.0)):
        with pytest.raises(ValueError, match="at most one"):
            g.Adam(**kw)
    for name in ("clipnorm", "global_clipnorm", "clipvalue"):
        for bad in (0.0, -1.0, float("nan"), float("inf"), 1e39, 1e-50):       # (the last two are inf / 0 as float32)
            with pytest.raises(ValueError, match=name):
                g.Adam(**{name: bad})
        opt = g.Adam(**{name: 0.25})
        assert [getattr(opt, k) for k in ("clipnorm", "global_clipnorm", "clipvalue")] == [0.25 if k == name else None for k in
                                                                                           ("clipnorm", "global_clipnorm", "clipvalue")]
        assert getattr(g.LossScaleOptimizer(opt), name) == 0.25                 # the wrapper forwards attributes
    opt = g.Adam()
    assert (opt.clipnorm, opt.global_clipnorm, opt.clipvalue) == (None, None, None)


def test_engine_hyper_parameters_carry_the_pair_only_when_set():
    hp = g.model.engine_hyper_parameters
    base = dict(beta_1=0.9, beta_2=0.999, epsilon=1e-7, base_lr=2e-5, warm_up=2000)
    assert hp(g.Adam(g.WarmUp(2e-5, 2000))) == base
    assert hp(g.model.default_optimizer()) == dict(base, warm_up=g.model.warm_up)
    assert hp(g.Adam(g.WarmUp(2e-5, 2000), clipnorm=1.5)) == dict(base, clip_mode=NORM, clip=1.5)
    assert hp(g.Adam(g.WarmUp(2e-5, 2000), global_clipnorm=2)) == dict(base, clip_mode=GLOBAL, clip=2.0)
    assert hp(g.LossScaleOptimizer(g.Adam(g.WarmUp(2e-5, 2000), clipvalue=0.5))) == dict(base, clip_mode=VALUE, clip=0.5)
    assert hp(g.Adam(g.WarmUp(2e-5, 2000), use_ema=True, clipvalue=0.5)) == dict(base, use_ema=True, ema_momentum=0.99, clip_mode=VALUE, clip=0.5)


def test_compile_passes_clipping_on_through_set_clipping():
    """Trainer.compile on an existing engine: set_clipping(...), never a plain attribute write; an optimizer without clipping
    switches it off; an engine that never clipped is not asked"""
    calls = []

    def set_clipping(**kw):
        calls.append(kw)
        eng.clip_mode = 0 if all(v is None for v in kw.values()) else 1

    eng = types.SimpleNamespace(ls_state=None, iterations=0, use_ema=False, set_clipping=set_clipping)
    tr = g.Trainer(types.SimpleNamespace(engine=eng))
    tr.compile(g.Adam(g.WarmUp(1e-4, 7)), g.identity)
    assert calls == [] and not hasattr(eng, "clip")
    tr.compile(g.Adam(g.WarmUp(1e-4, 7), global_clipnorm=1.0), g.identity)
    tr.compile(g.Adam(g.WarmUp(1e-4, 7), clipvalue=0.5), g.identity)
    tr.compile(g.Adam(g.WarmUp(1e-4, 7)), g.identity)
    tr.compile(g.Adam(g.WarmUp(1e-4, 7)), g.identity)
    none = dict(clipnorm=None, global_clipnorm=None, clipvalue=None)
    assert calls == [dict(none, global_clipnorm=1.0), dict(none, clipvalue=0.5), none] and eng.base_lr == 1e-4
    assert not hasattr(eng, "clip")                                # (the pair is never written as plain attributes)


def test_set_clipping_validates_and_switches():
    from gan_class_transfer2_amd.trainer_math import TrainerState

    class Stub(TrainerState):
        def __init__(self):
            pass

    eng = Stub()
    assert (eng.clip_mode, eng.clip) == (NONE, 0.0) and "clip_mode" not in eng.__dict__       # class-level defaults
    eng.set_clipping(clipnorm=0.5)
    assert (eng.clip_mode, eng.clip) == (NORM, 0.5)
    eng.set_clipping(global_clipnorm=3)
    assert (eng.clip_mode, eng.clip) == (GLOBAL, 3.0)
    eng.set_clipping(clipvalue=0.25)
    assert (eng.clip_mode, eng.clip) == (VALUE, 0.25)
    for kw in (dict(clipnorm=1.0, clipvalue=1.0), dict(clipnorm=0.0), dict(global_clipnorm=-2.0), dict(clipvalue=float("nan")),
               dict(clipvalue=float("inf"))):
        with pytest.raises(ValueError):
            eng.set_clipping(**kw)
        assert (eng.clip_mode, eng.clip) == (VALUE, 0.25)           # a refused call changes nothing
    eng.set_clipping()
    assert (eng.clip_mode, eng.clip) == (NONE, 0.0)
    eng._clip_forbidden = "driven by DataParallelStep"
    eng.set_clipping()                                              # switching off is always allowed
    with pytest.raises(ValueError, match="DataParallelStep"):
        eng.set_clipping(clipvalue=1.0)


# ---- the engines' call lists (no device: _lib.call is replaced by a recorder) ----------------------------------------------------
class _Calls:
    def __init__(self):
        self.log = []

    def __call__(self, name, *args):
        self.log.append((name, tuple(a.value if type(a) is g._lib.Slot else a for a in args)))


def _host_engine(monkeypatch, loss_scaled):
    """a UNetEngine with only the attributes the optimizer host logic reads, on a CPU arena of the smallest topology (the pattern of
    tests/test_ema_cpu.py::_host_engine)"""
    import torch
    from gan_class_transfer2_amd import engine as E, trainer_math as TM

    class Stub(E.UNetEngine):
        def __init__(self, **kw):
            self.__dict__.update(kw)

        def flush_deferred(self):
            pass

        def _stream(self):
            return 5

    calls = _Calls()
    monkeypatch.setattr(E, "call", calls)
    monkeypatch.setattr(TM, "call", calls)
    A = E.ParamArena(g.Topology(8, 16, 2), g.BF16, torch.device("cpu"))
    ls = torch.zeros(8, dtype=torch.int32) if loss_scaled else None
    eng = Stub(arena=A, dtype=g.BF16, ls_state=ls, _iterations=3, _pending=[], base_lr=1e-3, warm_up=0, beta_1=0.9, beta_2=0.999, epsilon=1e-7)
    return eng, A, calls


@pytest.mark.parametrize("loss_scaled", [False, True], ids=["plain", "loss_scaled"])
def test_apply_adam_call_lists_in_the_four_modes(monkeypatch, loss_scaled):
    eng, A, calls = _host_engine(monkeypatch, loss_scaled)
    ls_ptr = eng.ls_state.data_ptr() if loss_scaled else None
    alpha = 0.0 if loss_scaled else eng.adam_alpha()
    ptrs = lambda lo: (A._p.data_ptr() + 4 * lo, A._m.data_ptr() + 4 * lo, A._v.data_ptr() + 4 * lo, A.g.data_ptr() + 4 * lo,
                       A._shadow.data_ptr() + 2 * lo)
    hyper = (alpha, 0.9, 0.999, 1e-7)

    def step():
        """what _step_body does behind the reverse pass of a non-fused step"""
        del calls.log[:]
        if not eng._clip_by_norm():
            eng.check_finite()
        eng.apply_adam()
        return list(calls.log)

    # off: the call list of before - no new symbol, no table
    check = [("gct2_scale_check_finite", (A.g.data_ptr(), A.total, ls_ptr, 5))] if loss_scaled else []
    plain = check + [("gct2_adam_keras_multi", ptrs(0) + (g.BF16, A.total) + hyper + (1.0, ls_ptr, 0, 5))]
    assert step() == plain and eng._clip_table is None
    # clipvalue: one clipped launch over [0, total); the finite check stays; still nothing allocated
    eng.set_clipping(clipvalue=0.5)
    assert step() == check + [("gct2_adam_keras_clipped", ptrs(0) + (g.BF16, A.total) + hyper + (1.0, ls_ptr, VALUE, 0.5, None, 5))]
    assert eng._clip_table is None
    # the table: one segment per tensor, in arena order, without the alignment padding
    segs = sorted((o, A.numel(n)) for n, o in A.offsets.items())
    assert len(segs) == len(A.shapes) == 10 and all(b % 64 == 0 for b, _ in segs)
    assert any(c % 64 for _, c in segs) and sum(c for _, c in segs) < A.total                 # (there IS padding to leave out)
    # global_clipnorm: the reduction (which sets found_inf: no gct2_scale_check_finite), then one launch reading sumsq[nseg]
    eng.set_clipping(global_clipnorm=2.0)
    log = step()
    table, nseg, npart, partials, sumsq, host_segs = eng._clip_table
    assert host_segs == segs and nseg == 10 and npart == sum(K.partial_counts(segs)) == partials.numel() and sumsq.numel() == 11
    assert table.view(-1, 3).tolist() == [[b, c, sum(K.partial_counts(segs[:s]))] for s, (b, c) in enumerate(segs)]
    reduce = ("gct2_grad_sumsq", (A.g.data_ptr(), table.data_ptr(), 10, npart, 1.0, ls_ptr, partials.data_ptr(), sumsq.data_ptr(), 5))
    assert log == [reduce, ("gct2_adam_keras_clipped", ptrs(0) + (g.BF16, A.total) + hyper + (1.0, ls_ptr, GLOBAL, 2.0, sumsq.data_ptr() + 80, 5))]
    # clipnorm: the reduction, then one launch per tensor over exactly its elements with its own sum; the table is built once
    eng.set_clipping(clipnorm=0.25)
    log = step()
    assert eng._clip_table[0] is table
    assert log == [reduce] + [("gct2_adam_keras_clipped", ptrs(b) + (g.BF16, c) + hyper + (1.0, ls_ptr, NORM, 0.25, sumsq.data_ptr() + 8 * s, 5))
                              for s, (b, c) in enumerate(segs)]
    assert "gct2_scale_check_finite" not in [n for n, _ in log]
    # a sub-range: refused in the norm modes, clipped per element under clipvalue, and the data-parallel mean reaches the reduction
    lo, hi = A.layer_ranges["U1"]
    for kw in (dict(clipnorm=0.25), dict(global_clipnorm=2.0)):
        eng.set_clipping(**kw)
        del calls.log[:]
        with pytest.raises(ValueError, match="norm"):
            eng.apply_adam(lo, hi)
        with pytest.raises(ValueError, match="norm"):
            eng.apply_adam(0, hi)
        assert calls.log == []
    eng.apply_adam(grad_div=4.0, stream=9)
    assert calls.log[0] == ("gct2_grad_sumsq", reduce[1][:4] + (0.25,) + reduce[1][5:8] + (9,)) and calls.log[1][1][11] == 0.25
    eng.set_clipping(clipvalue=0.5)
    del calls.log[:]
    eng.apply_adam(lo, hi, grad_div=2.0)
    assert calls.log == [("gct2_adam_keras_clipped", ptrs(lo) + (g.BF16, hi - lo) + hyper + (0.5, ls_ptr, VALUE, 0.5, None, 5))]
    # off again: the call list of before
    eng.set_clipping()
    assert step() == plain


def test_plan_key_carries_the_pair():
    import inspect
    from gan_class_transfer2_amd import engine as E
    src = inspect.getsource(E.UNetEngine._plan_key)
    assert "self.clip_mode" in src and "float(self.clip)" in src


# ---- the numpy restatement on its corner cases --------------------------------------------------------------------------------------
def test_restatement_corner_cases():
    F = np.float32
    gp = np.array([-3.0, -0.5, 0.0, 0.25, np.nan, 7.0, np.inf, -np.inf], dtype=F)
    out = K.clip(gp, VALUE, 0.5)
    assert np.array_equal(out[[0, 1, 2, 3, 5, 6, 7]], np.array([-0.5, -0.5, 0.0, 0.25, 0.5, 0.5, -0.5], dtype=F)) and np.isnan(out[4])
    assert out.dtype == F
    # GLOBAL_NORM at nrm = 0: scale = clip * (1 / clip) - min(inf, 1 / clip) - which is not 1 for every clip
    for c in (0.3, 3.0, 41.0):
        x = np.array([1.0, -2.0], dtype=F)
        want = x * (F(c) * (F(1.0) / F(c)))
        assert np.array_equal(K.clip(x, GLOBAL, c, 0.0), want)
    assert F(41.0) * (F(1.0) / F(41.0)) != F(1.0)                    # (... so the case is not vacuous)
    # a non-finite norm gives NaN everywhere
    for ss in (np.inf, np.nan, 1e300):                               # sqrt(1e300) = 1e150 is inf as float32
        assert np.isnan(K.clip(np.array([1.0, 0.0, -2.0], dtype=F), GLOBAL, 1.0, ss)).all()
    # below the threshold the global scale is clip * (1 / clip), above it clip * (1 / nrm)
    x = np.array([3.0, 4.0], dtype=F)
    assert np.array_equal(K.clip(x, GLOBAL, 10.0, 25.0), x * (F(10.0) * (F(1.0) / F(10.0))))
    assert np.array_equal(K.clip(x, GLOBAL, 1.0, 25.0), x * (F(1.0) * (F(1.0) / F(5.0))))
    # NORM: an all-zero tensor (sumsq = 0 -> l2 = 1) returns zeros; inside the threshold g * clip / clip; outside g * clip / l2
    z = np.zeros(5, dtype=F)
    assert np.array_equal(K.clip(z, NORM, 0.5, 0.0), z) and np.array_equal(K.clip(z, NORM, 2.0, 0.0), z)
    assert np.array_equal(K.clip(x, NORM, 10.0, 25.0), (x * F(10.0)) / F(10.0))
    assert np.array_equal(K.clip(x, NORM, 1.0, 25.0), (x * F(1.0)) / F(5.0))
    assert np.array_equal(K.clip(x, NONE), x)
    # the reduction: exact inputs sum exactly in any order, and the total is the sum of the segment sums
    segs, total = K.layout()
    assert K.assert_exact_bound(segs) < 1 << 53
    rng = np.random.default_rng(1)
    buf = K.poisoned(lambda s, n: K.exact_values(rng, n), segs, total)
    assert np.isnan(buf[:K.GUARD]).all() and np.isnan(buf[-K.GUARD:]).all() and float(np.abs(buf[~np.isnan(buf)]).max()) <= 2.0 ** 10
    ss = K.segment_sumsq(buf, segs)
    for s, (b, c) in enumerate(segs):
        sq = (buf[b:b + c].astype(np.float64) * 2.0 ** 4) ** 2                      # integers
        assert ss[s] == float(int(sq[::-1].sum())) * 2.0 ** -8 == float(sum(int(v) for v in sq)) * 2.0 ** -8
    assert ss[-1] == ss[:-1].sum() and np.isfinite(ss).all()
    # scaling by powers of two keeps it exact
    assert K.segment_sumsq(K.scaled(buf, 0.5, 2.0 ** -7), segs)[-1] == ss[-1] * 2.0 ** -16


def test_restated_adam_is_the_oracles():
    """the float32 Adam of clip_cases against oracle.denoiser_oracle.keras_adam_step (same formula, its own evaluation order):
    equal to a few float32 roundings"""
    from oracle import denoiser_oracle as O
    import math
    cfg = O.OracleConfig()
    rng = np.random.default_rng(2)
    n = 1000
    p, gr = rng.standard_normal(n).astype(np.float32), (rng.standard_normal(n) * 1e-3).astype(np.float32)
    m, v = (rng.standard_normal(n) * 1e-3).astype(np.float32), (rng.random(n) * 1e-6).astype(np.float32)
    k = 5
    alpha = O.warmup_lr(k, cfg.base_lr, cfg.warm_up) * math.sqrt(1 - cfg.beta_2 ** (k + 1)) / (1 - cfg.beta_1 ** (k + 1))
    want = O.keras_adam_step(p, gr, m, v, k, cfg)
    got = K.adam(p, m, v, gr, alpha, cfg.beta_1, cfg.beta_2, cfg.epsilon)
    for a, b in zip(got, want):
        assert a.dtype == np.float32 and np.allclose(a, b, rtol=1e-5, atol=0)
