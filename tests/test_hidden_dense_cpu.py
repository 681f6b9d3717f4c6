"""The hidden Dense(pixel_size, relu) layer in front of the head (train.py:195-197) and the head's initializer (train.py:199), the parts
that need no GPU: the three C entry points and their rejection contract (the ORDER of the checks is part of the interface, include/gct2.h),
the scratch query, the module switches, the shapes and Glorot limits of the new tensors.

The rejection table runs like tests/test_capi_contract_cpu.py's: in a fresh child process (this file as a script) whose environment
hides the GPUs, with fake aligned addresses, and only when gct2_device_check() says GCT2_ENODEV there."""
import ctypes
import importlib.util
import json
import math
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, BF16, F16 = 0, 1, 2
OK, EINVAL, ENODEV = 0, 1, 3
P = 4096                    # a fake, 16-byte aligned device address; no row lets a call get as far as reading it
NEW = ("gct2_dense2_fwd", "gct2_dense2_bwd", "gct2_dense2_scratch")
ROW = 67 * 128 + 128 + 128 * 3 + 3 + 1      # one partial row [dw1 | db1 | dw2 | db2] of the reference head, padded to a multiple of 4


def _args(defaults, over):
    unknown = set(over) - set(defaults)
    assert not unknown, unknown
    return list({**defaults, **over}.values())


def fwd(**o):           # gct2_dense2_fwd, valid arguments in prototype order
    return _args(dict(ctx=None, dtype=BF16, x=P, ldx=72, w1=P, b1=P, w2=P, b2=P, y=P, M=432, Cin=67, Chid=128, Cout=3, stream=None), o)


def bwd(**o):           # gct2_dense2_bwd; 1 << 22 floats of scratch cover every shape of the table that gets that far
    return _args(dict(ctx=None, dtype=BF16, x=P, ldx=72, w1=P, b1=P, w2=P, dy=P, dx=P, lddx=64, dw1=P, db1=P, dw2=P, db2=P, scratch=P,
                      scratch_floats=1 << 22, M=432, Cin=67, Chid=128, Cout=3, Cmask=64, accumulate=0, stream=None), o)


def _rows(name, build, nulls):
    """the checks both launching calls share, in their order: dtype, NULL, dims, Cout, ldx, ..., M, weight counts, plain-tile limits"""
    fn = "gct2_" + name
    dim = lambda **kw: f"{name}: non-positive dimension (M={kw.get('M', 432)} Cin={kw.get('Cin', 67)} Chid={kw.get('Chid', 128)})"
    big = dict(Cin=1 << 16, ldx=1 << 16, Chid=1 << 15)        # 2^31 kernel entries
    rows = [(fn, build(dtype=7), EINVAL, f"{name}: unknown dtype 7"), (fn, build(dtype=-1), EINVAL, f"{name}: unknown dtype -1")]
    rows += [(fn, build(**{k: None}), EINVAL, f"{name}: null pointer ({', '.join(nulls)})") for k in nulls]
    rows += [(fn, build(**kw), EINVAL, dim(**kw)) for kw in (dict(M=0), dict(M=-5), dict(Cin=0), dict(Chid=-1))]
    rows += [(fn, build(Cout=0), EINVAL, f"{name}: Cout=0 outside 1..4"), (fn, build(Cout=5), EINVAL, f"{name}: Cout=5 outside 1..4"),
             (fn, build(ldx=66), EINVAL, f"{name}: ldx=66 smaller than Cin=67"),
             (fn, build(M=(1 << 31) - 1), EINVAL, f"{name}: M=2147483647 too large for 32-bit pixel indices"),
             (fn, build(M=(1 << 31) - 64), EINVAL, f"{name}: M=2147483584 too large for 32-bit pixel indices"),
             (fn, build(**big), EINVAL, f"{name}: Cin*Chid or Chid*Cout too large for 32-bit weight indices"),
             (fn, build(Chid=257), EINVAL, f"{name}: Cin=67 / Chid=257 beyond 256, the plain kernel's LDS tile"),
             (fn, build(Cin=300, ldx=304), EINVAL, f"{name}: Cin=300 / Chid=128 beyond 256, the plain kernel's LDS tile"),
             # two mistakes: the earlier check names the call
             (fn, build(dtype=7, x=None), EINVAL, f"{name}: unknown dtype 7"),
             (fn, build(w1=None, M=0), EINVAL, f"{name}: null pointer ({', '.join(nulls)})"),
             (fn, build(Chid=0, Cout=9), EINVAL, dim(Chid=0)),
             (fn, build(Cout=5, ldx=1), EINVAL, f"{name}: Cout=5 outside 1..4"),
             (fn, build(ldx=66, M=(1 << 31) - 1), EINVAL, f"{name}: ldx=66 smaller than Cin=67"),
             (fn, build(M=(1 << 31) - 1, Chid=257), EINVAL, f"{name}: M=2147483647 too large for 32-bit pixel indices")]
    return rows


CASES = (_rows("dense2_fwd", fwd, ("x", "w1", "b1", "w2", "b2", "y"))
         + _rows("dense2_bwd", bwd, ("x", "w1", "b1", "w2", "dy", "dw1", "db1", "dw2", "db2", "scratch"))
         + [("gct2_dense2_bwd", bwd(Cmask=68), EINVAL, "dense2_bwd: Cmask=68 outside 0..Cin or lddx=64 smaller than it"),
            ("gct2_dense2_bwd", bwd(Cmask=-1), EINVAL, "dense2_bwd: Cmask=-1 outside 0..Cin or lddx=64 smaller than it"),
            ("gct2_dense2_bwd", bwd(lddx=63), EINVAL, "dense2_bwd: Cmask=64 outside 0..Cin or lddx=63 smaller than it"),
            # (the Cmask check stands behind ldx and in front of the size checks)
            ("gct2_dense2_bwd", bwd(ldx=66, Cmask=68), EINVAL, "dense2_bwd: ldx=66 smaller than Cin=67"),
            ("gct2_dense2_bwd", bwd(Cmask=68, Chid=257), EINVAL, "dense2_bwd: Cmask=68 outside 0..Cin or lddx=64 smaller than it"),
            ("gct2_dense2_bwd", bwd(scratch=P + 4), EINVAL, "dense2_bwd: scratch must be 16-byte aligned"),
            ("gct2_dense2_bwd", bwd(scratch=P + 4, scratch_floats=0), EINVAL, "dense2_bwd: scratch must be 16-byte aligned"),
            ("gct2_dense2_bwd", bwd(scratch_floats=0), EINVAL, f"dense2_bwd: 0 floats of scratch, this shape needs {27 * ROW} (gct2_dense2_scratch)"),
            ("gct2_dense2_bwd", bwd(scratch_floats=27 * ROW - 1), EINVAL,
             f"dense2_bwd: {27 * ROW - 1} floats of scratch, this shape needs {27 * ROW} (gct2_dense2_scratch)"),
            ("gct2_dense2_bwd", bwd(Chid=257, scratch_floats=0), EINVAL, "dense2_bwd: Cin=67 / Chid=257 beyond 256, the plain kernel's LDS tile"),
            ("gct2_dense2_scratch", [432, 67, 128, 3, None], EINVAL, "dense2_scratch: null output pointer"),
            ("gct2_dense2_scratch", [0, 67, 128, 3, None], EINVAL, "dense2_scratch: null output pointer")])


def _load_lib():
    spec = importlib.util.spec_from_file_location("gct2_lib", os.path.join(ROOT, "gan-class-transfer2_amd", "_lib.py"))
    L = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(L)
    return L


def _child():
    L = _load_lib()
    lib = L.load()
    out = {"device": lib.gct2_device_check(), "results": []}
    if out["device"] == ENODEV:
        for fn, args, _code, _text in CASES:
            code = getattr(lib, fn)(*args)
            out["results"].append([code, lib.gct2_last_error().decode()])
    print(json.dumps(out))


def test_rejected_calls_return_their_codes_and_texts():
    env = dict(os.environ)
    env.update(HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    if out["device"] != ENODEV:
        pytest.skip(f"a device is visible to the child process (gct2_device_check() = {out['device']}): fake pointers are not sent to it")
    assert len(out["results"]) == len(CASES) >= 60
    wrong = [(i, fn, got, [code, text]) for i, ((fn, _a, code, text), got) in enumerate(zip(CASES, out["results"])) if got != [code, text]]
    assert not wrong, wrong


def test_library_exports_and_declares_the_three_entry_points():
    import gan_class_transfer2_amd as g
    L = g._lib
    lib = L.load()
    raw = ctypes.CDLL(L.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "gct2.h")).read()
    for name in NEW:
        assert hasattr(raw, name) and name in L.SIGNATURES, name
        assert re.search(r"\bint " + name + r"\(", header), name
    assert lib.gct2_abi_version() == L.ABI_VERSION == 17              # additions change no signature
    assert "v17 + gct2_dense2_fwd, gct2_dense2_bwd, gct2_dense2_scratch (additive)" in header
    # the constants the binding exposes are the header's
    assert int(re.search(r"#define GCT2_DENSE2_FAST_PIXELS (\d+)", header).group(1)) == L.DENSE2_FAST_PIXELS
    assert int(re.search(r"#define GCT2_DENSE2_PLAIN_MAX (\d+)", header).group(1)) == L.DENSE2_PLAIN_MAX
    # argument counts of the prototypes in the issue: 14, 5, 23
    assert [len(L.SIGNATURES[n]) for n in NEW] == [14, 23, 5]
    assert "gct2_dense2_fwd" in L.PLANNABLE and "gct2_dense2_bwd" in L.PLANNABLE and "gct2_dense2_scratch" not in L.PLANNABLE
    # a step plan can hold the two launching calls, not the host-only query
    plan = L.Plan()
    arr = (ctypes.c_uint64 * 5)()
    assert lib.gct2_plan_add_call(plan.handle, b"gct2_dense2_scratch", arr, 5, None) == EINVAL and b"not an entry point" in lib.gct2_last_error()
    for name in NEW[:2]:
        n = len(L.SIGNATURES[name])
        arr = (ctypes.c_uint64 * n)()
        assert lib.gct2_plan_add_call(plan.handle, name.encode(), arr, n, None) == OK, name
        assert lib.gct2_plan_add_call(plan.handle, name.encode(), arr, n - 1, None) == EINVAL


def test_scratch_query_is_monotone_and_never_zero():
    import gan_class_transfer2_amd as g
    lib = g._lib.load()
    need = ctypes.c_size_t(0)
    last = 0
    for M in (1, 2, 15, 16, 17, 37, 64, 65, 165, 432, 8191, 8192, 8193, 1 << 20, 1 << 26):
        assert lib.gct2_dense2_scratch(M, 67, 128, 3, ctypes.byref(need)) == OK, M
        assert need.value >= last and need.value > 0 and need.value % ROW == 0, (M, need.value)
        last = need.value
    assert last == 512 * ROW                                         # the number of partial rows stops growing at 512 work-groups
    assert lib.gct2_dense2_scratch(432, 67, 128, 3, ctypes.byref(need)) == OK and need.value == 27 * ROW       # ceil(432 / 16) rows
    for cin, chid, cout in ((11, 8, 1), (1, 1, 4), (256, 256, 4)):
        assert lib.gct2_dense2_scratch(1, cin, chid, cout, ctypes.byref(need)) == OK
        assert need.value == (cin * chid + chid + chid * cout + cout + 3) // 4 * 4
    assert lib.gct2_dense2_scratch(432, 67, 128, 5, ctypes.byref(need)) == EINVAL
    assert lib.gct2_last_error().decode() == "dense2_scratch: Cout=5 outside 1..4"
    assert lib.gct2_dense2_scratch(0, 67, 128, 3, ctypes.byref(need)) == EINVAL
    assert lib.gct2_dense2_scratch(432, 67, 257, 3, ctypes.byref(need)) == EINVAL


def test_configure_accepts_and_validates_the_switches():
    import gan_class_transfer2_amd as g
    M = g.model
    assert M.hidden_dense is False and M.head_initializer == "glorot_uniform"
    try:
        g.configure(hidden_dense=True, head_initializer="zeros")
        assert M.hidden_dense is True and M.head_initializer == "zeros"
        for bad in ("ones", "Zeros", None, 0):
            with pytest.raises(ValueError, match="head_initializer"):
                g.configure(head_initializer=bad)
        assert M.head_initializer == "zeros"                         # a refused value changes nothing
        with pytest.raises(ValueError, match="hidden_dense"):
            g.configure(hidden_dense="yes")
        assert M.hidden_dense is True
    finally:
        g.configure(hidden_dense=False, head_initializer="glorot_uniform")


def test_head_options_are_checked_before_anything_is_built():
    from gan_class_transfer2_amd.trainer_math import HEAD_INITIALIZERS, check_head_options, check_hidden_marker
    assert HEAD_INITIALIZERS == ("glorot_uniform", "zeros")
    check_head_options("UNetEngine", True, False, "zeros")
    check_head_options("UNetEngine", False, True, "glorot_uniform")
    with pytest.raises(ValueError, match="hidden_dense.*timestep_heads"):
        check_head_options("UNetEngine", True, True, "glorot_uniform")
    with pytest.raises(ValueError, match="head_initializer"):
        check_head_options("VariantEngine", False, False, "ones")
    check_hidden_marker({"hidden_dense": [128]}, True)
    check_hidden_marker({}, False)
    for sd, on in (({}, True), ({"hidden_dense": [128]}, False)):
        with pytest.raises(ValueError, match="nothing is loaded"):
            check_hidden_marker(sd, on)


def test_shapes_and_glorot_limits_of_the_new_tensors():
    import gan_class_transfer2_amd as g
    from gan_class_transfer2_amd.trainer_math import glorot_limit
    topo = g.Topology(128, 512, 6)
    off, on = topo.param_shapes(), topo.param_shapes(3, True)
    assert "dense_hidden.w" not in off and off["dense.w"] == (67, 3)
    assert on["dense_hidden.w"] == (67, 128) and on["dense_hidden.b"] == (128,) and on["dense.w"] == (128, 3) and on["dense.b"] == (3,)
    assert {k: v for k, v in on.items() if not k.startswith("dense")} == {k: v for k, v in off.items() if not k.startswith("dense")}
    assert glorot_limit(on["dense_hidden.w"]) == math.sqrt(6.0 / (67 + 128)) and glorot_limit(on["dense.w"]) == math.sqrt(6.0 / (128 + 3))
    small = g.Topology(8, 32, 2).param_shapes(3, True)
    assert small["dense_hidden.w"] == (4 + 3, 8) and small["dense.w"] == (8, 3)


def test_eager_dense_layer_takes_the_relu_activation_only():
    import gan_class_transfer2_amd as g
    D = g.model.Dense
    assert D(8, activation="relu").activation == "relu" and D(3).activation is None
    for bad in ("tanh", "ReLU", True):
        with pytest.raises(ValueError, match="activation"):
            D(8, activation=bad)
    with pytest.raises(ValueError, match="activation"):
        D(8, use_bias=False, activation="relu")
    with pytest.raises(ValueError, match="kernel_initializer"):
        D(3, kernel_initializer="ones")


def test_data_parallel_wrappers_name_both_sides_in_their_refusal():
    from gan_class_transfer2_amd import distributed

    class Eng:
        hidden_dense = True
    for who in ("DataParallelStep", "ShardedDataParallelStep"):
        with pytest.raises(ValueError, match=who + ".*hidden_dense"):
            distributed._refuse_hidden_dense(Eng(), who)
    Eng.hidden_dense = False
    distributed._refuse_hidden_dense(Eng(), "DataParallelStep")


if __name__ == "__main__":
    _child()
