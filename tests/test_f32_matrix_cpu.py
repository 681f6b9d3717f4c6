"""fp32 matrix-core switch (gct2_ctx_set_f32_math): the host-side surface, no GPU needed."""
import ctypes

import gan_class_transfer2_amd as g
from gan_class_transfer2_amd import _lib


def test_setter_exported_and_bound():
    lib = _lib.load()
    assert "gct2_ctx_set_f32_math" in _lib.SIGNATURES
    assert _lib.SIGNATURES["gct2_ctx_set_f32_math"] == [ctypes.c_void_p, ctypes.c_int]
    assert hasattr(lib, "gct2_ctx_set_f32_math")
    assert (_lib.F32_MATH_DIRECT, _lib.F32_MATH_MFMA) == (0, 1)


def test_setter_rejects_unknown_modes_and_null_ctx():
    lib = _lib.load()
    c = _lib.Context()
    for mode in (2, -1):
        assert lib.gct2_ctx_set_f32_math(c.handle, mode) == 1          # GCT2_EINVAL
    assert lib.gct2_ctx_set_f32_math(None, _lib.F32_MATH_MFMA) == 1
    for mode in (_lib.F32_MATH_MFMA, _lib.F32_MATH_DIRECT):
        assert lib.gct2_ctx_set_f32_math(c.handle, mode) == 0


def test_context_setter_bumps_version():
    c = _lib.Context()
    v = c.version
    c.set_f32_math(_lib.F32_MATH_MFMA)
    assert c.version > v and c.f32_math == _lib.F32_MATH_MFMA
    other = _lib.Context()
    other.mirror(c)
    assert other.f32_math == _lib.F32_MATH_MFMA
    v = c.version
    try:
        c.set_f32_math(2)
        raised = False
    except _lib.Gct2Error:
        raised = True
    assert raised and c.f32_math == _lib.F32_MATH_MFMA


def test_model_knob_off_by_default():
    assert g.model.f32_matrix_cores is False
