"""Per-timestep heads (train.py:199, 203, 211-214: Dense(3 * steps), Reshape, tf.gather by t - 1), the parts that need no GPU: the module
switch, the host check of the timesteps, the three C entry points and their rejection contract.

The rejection table runs like tests/test_capi_contract_cpu.py's: in a fresh child process (this file as a script) whose environment
hides the GPUs, with fake aligned addresses, and only when gct2_device_check() says GCT2_ENODEV there."""
import ctypes
import importlib.util
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, BF16, F16 = 0, 1, 2
OK, EINVAL, ENODEV = 0, 1, 3
P = 4096                    # a fake, 16-byte aligned device address; no row lets a call get as far as reading it
NEW = ("gct2_dense_steps_fwd", "gct2_dense_steps_bwd", "gct2_dense_steps_scratch")


def _args(defaults, over):
    unknown = set(over) - set(defaults)
    assert not unknown, unknown
    return list({**defaults, **over}.values())


def fwd(**o):           # gct2_dense_steps_fwd, valid arguments in prototype order
    return _args(dict(ctx=None, dtype=BF16, x=P, ldx=72, w=P, b=P, t_int=P, y=P, B=3, HW=144, Cin=67, Cout=3, steps=200, stream=None), o)


def bwd(**o):           # gct2_dense_steps_bwd; 1 << 20 floats of scratch cover every shape of the table that gets that far
    return _args(dict(ctx=None, dtype=BF16, x=P, ldx=72, w=P, t_int=P, dy=P, dx=P, lddx=64, dw=P, db=P, scratch=P, scratch_floats=1 << 20,
                      B=3, HW=144, Cin=67, Cout=3, steps=200, Cmask=64, accumulate=0, stream=None), o)


def _rows(name, build, nulls):
    fn = "gct2_" + name
    dim = lambda **kw: f"{name}: non-positive dimension (B={kw.get('B', 3)} HW={kw.get('HW', 144)} Cin={kw.get('Cin', 67)} steps={kw.get('steps', 200)})"
    rows = [(fn, build(dtype=7), EINVAL, f"{name}: unknown dtype 7"), (fn, build(dtype=-1), EINVAL, f"{name}: unknown dtype -1")]
    rows += [(fn, build(**{k: None}), EINVAL, f"{name}: null pointer ({', '.join(nulls)})") for k in nulls]
    rows += [(fn, build(**kw), EINVAL, dim(**kw)) for kw in (dict(B=0), dict(HW=0), dict(Cin=-1), dict(steps=0))]
    rows += [(fn, build(Cout=0), EINVAL, f"{name}: Cout=0 outside 1..4"), (fn, build(Cout=5), EINVAL, f"{name}: Cout=5 outside 1..4"),
             (fn, build(ldx=66), EINVAL, f"{name}: ldx=66 smaller than Cin=67"),
             (fn, build(B=1 << 15, HW=1 << 16), EINVAL, f"{name}: B*HW too large for 32-bit pixel indices"),
             (fn, build(Cin=1 << 14, ldx=1 << 14, steps=1 << 15, Cout=4), EINVAL, f"{name}: Cin*steps*Cout too large for 32-bit weight indices"),
             (fn, build(B=1 << 16), EINVAL, f"{name}: B=65536 / steps=200 beyond 65535 (one grid row per image / per slice)"),
             # two mistakes: the earlier check names the call
             (fn, build(dtype=7, x=None), EINVAL, f"{name}: unknown dtype 7"),
             (fn, build(w=None, B=0), EINVAL, f"{name}: null pointer ({', '.join(nulls)})"),
             (fn, build(Cout=5, ldx=1), EINVAL, f"{name}: Cout=5 outside 1..4")]
    return rows


CASES = (_rows("dense_steps_fwd", fwd, ("x", "w", "t_int", "y"))
         + _rows("dense_steps_bwd", bwd, ("x", "w", "t_int", "dy", "dw", "scratch"))
         + [("gct2_dense_steps_bwd", bwd(scratch_floats=0), EINVAL, "dense_steps_bwd: 0 floats of scratch, this shape needs 1224 (gct2_dense_steps_scratch)"),
            ("gct2_dense_steps_bwd", bwd(scratch_floats=1223), EINVAL, "dense_steps_bwd: 1223 floats of scratch, this shape needs 1224 (gct2_dense_steps_scratch)"),
            ("gct2_dense_steps_bwd", bwd(scratch=P + 4), EINVAL, "dense_steps_bwd: scratch must be 16-byte aligned"),
            ("gct2_dense_steps_bwd", bwd(Cmask=68), EINVAL, "dense_steps_bwd: Cmask=68 outside 0..Cin or lddx=64 smaller than it"),
            ("gct2_dense_steps_bwd", bwd(lddx=63), EINVAL, "dense_steps_bwd: Cmask=64 outside 0..Cin or lddx=63 smaller than it"),
            ("gct2_dense_steps_bwd", bwd(Cin=1024, ldx=1024, Cmask=0), EINVAL, "dense_steps_bwd: (Cin+1)*Cout = 3075 exceeds 2048"),
            ("gct2_dense_steps_bwd", bwd(dtype=F32, Cin=400, ldx=400, Cout=1, Cmask=0), EINVAL, "dense_steps_bwd: Cin=400 too large for the LDS tile")])


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
    assert len(out["results"]) == len(CASES) >= 40
    wrong = [(i, fn, got, [code, text]) for i, ((fn, _a, code, text), got) in enumerate(zip(CASES, out["results"])) if got != [code, text]]
    assert not wrong, wrong


def test_library_exports_the_three_entry_points():
    import gan_class_transfer2_amd as g
    L = g._lib
    lib = L.load()
    raw = ctypes.CDLL(L.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name) and name in L.SIGNATURES, name
    assert lib.gct2_abi_version() == L.ABI_VERSION == 17              # additions change no signature
    assert "gct2_dense_steps_fwd" in L.PLANNABLE and "gct2_dense_steps_bwd" in L.PLANNABLE and "gct2_dense_steps_scratch" not in L.PLANNABLE
    # a step plan can hold the two launching calls, not the host-only query
    plan = L.Plan()
    arr = (ctypes.c_uint64 * 5)()
    assert lib.gct2_plan_add_call(plan.handle, b"gct2_dense_steps_scratch", arr, 5, None) == EINVAL and b"not an entry point" in lib.gct2_last_error()
    for name in NEW[:2]:
        n = len(L.SIGNATURES[name])
        arr = (ctypes.c_uint64 * n)()
        assert lib.gct2_plan_add_call(plan.handle, name.encode(), arr, n, None) == OK, name
        assert lib.gct2_plan_add_call(plan.handle, name.encode(), arr, n - 1, None) == EINVAL


def test_scratch_query():
    import gan_class_transfer2_amd as g
    lib = g._lib.load()
    need = ctypes.c_size_t(0)
    assert lib.gct2_dense_steps_scratch(3, 144, 67, 3, ctypes.byref(need)) == OK and need.value > 0
    # one partial row of (Cin + 1) * Cout floats per (image, 128-pixel tile): 3 images x 2 tiles x 204
    assert need.value == 3 * 2 * 204
    assert lib.gct2_dense_steps_scratch(3, 144, 67, 5, ctypes.byref(need)) == EINVAL
    assert lib.gct2_last_error().decode() == "dense_steps_scratch: Cout=5 outside 1..4"
    assert lib.gct2_dense_steps_scratch(3, 144, 67, 3, None) == EINVAL
    assert lib.gct2_dense_steps_scratch(0, 144, 67, 3, ctypes.byref(need)) == EINVAL
    # the number of rows per image stops growing once the grid is full: never more than 2048 rows in all (plus one per image)
    assert lib.gct2_dense_steps_scratch(64, 128 * 128, 67, 3, ctypes.byref(need)) == OK and need.value == 64 * 32 * 204


def test_configure_accepts_the_switch():
    import gan_class_transfer2_amd as g
    M = g.model
    assert M.timestep_heads is False
    try:
        g.configure(timestep_heads=True)
        assert M.timestep_heads is True
    finally:
        g.configure(timestep_heads=False)


def test_check_timesteps_accepts():
    import numpy as np
    import torch
    from gan_class_transfer2_amd.trainer_math import check_timesteps
    steps = 200
    assert check_timesteps(1, 3, steps) == [1, 1, 1] and check_timesteps(steps, 2, steps) == [steps, steps]
    assert check_timesteps([1, steps, 7], 3, steps) == [1, steps, 7]
    assert check_timesteps(torch.tensor([[[[5]]], [[[6]]]]).reshape(-1), 2, steps) == [5, 6]         # [B,1,1,1] of Trainer.call, flattened
    assert check_timesteps(torch.tensor([9]), 4, steps) == [9] * 4                                   # [1] of log_sample: broadcast
    assert check_timesteps(np.array([3, 4], dtype=np.int64), 2, steps) == [3, 4]
    assert check_timesteps(np.int32(8), 1, steps) == [8]
    assert all(type(v) is int for v in check_timesteps(torch.tensor([2, 3], dtype=torch.int32), 2, steps))


@pytest.mark.parametrize("bad, batch", [(0, 1), (201, 1), ([1, 2], 3), ([1, 2, 3, 4], 3), (1.0, 1), ([1, 2.5], 2), (True, 1), (None, 1), ("3", 1),
                                        ([1, 0, 3], 3), ([1, 201], 2), ([], 2)])
def test_check_timesteps_rejects(bad, batch):
    from gan_class_transfer2_amd.trainer_math import check_timesteps
    with pytest.raises(ValueError):
        check_timesteps(bad, batch, 200)


def test_check_timesteps_rejects_float_tensors():
    import numpy as np
    import torch
    from gan_class_transfer2_amd.trainer_math import check_timesteps
    for bad in (torch.tensor([1.0]), torch.tensor([True]), np.array([1.0]), torch.tensor([0]), torch.tensor([201]), torch.tensor([1, 2])):
        with pytest.raises(ValueError):
            check_timesteps(bad, 3, 200)


def test_head_shapes_and_glorot_limit():
    import math
    import gan_class_transfer2_amd as g
    from gan_class_transfer2_amd.trainer_math import glorot_limit
    topo = g.Topology(128, 512, 6)
    assert topo.param_shapes()["dense.w"] == (67, 3) and topo.param_shapes()["dense.b"] == (3,)
    shp = topo.param_shapes(600)
    assert shp["dense.w"] == (67, 600) and shp["dense.b"] == (600,)
    assert {k: v for k, v in shp.items() if not k.startswith("dense.")} == {k: v for k, v in topo.param_shapes().items() if not k.startswith("dense.")}
    assert glorot_limit(shp["dense.w"]) == math.sqrt(6.0 / (67 + 600))


if __name__ == "__main__":
    _child()
