"""fp32 matrix cores on the stride-1 convolutions and the variant networks: the host-side surface, no GPU needed."""
import inspect

from gan_class_transfer2_amd import _lib

F32 = 0


def test_variant_engine_takes_the_f32_matrix_switch():
    from gan_class_transfer2_amd.variants import VariantEngine
    params = inspect.signature(VariantEngine).parameters
    assert "f32_matrix" in params and params["f32_matrix"].default is False


def test_s1_entry_points_check_their_arguments_before_the_f32_matrix_route():
    """in F32_MATH_MFMA mode the stride-1 entry points still reject an even kernel size, one above 7 and ld < C with GCT2_EINVAL
    before anything is launched (nothing in the launch log): the matrix-core route sits behind the existing checks.  The device
    pointers are fake addresses that these paths never dereference."""
    lib = _lib.load()
    c = _lib.Context()
    c.set_f32_math(_lib.F32_MATH_MFMA)
    c.log_launches(True)
    P = 4096
    B, H, W, Cin, Cout = 1, 4, 4, 8, 8
    for ks, ld in ((2, Cin), (9, Cin), (0, Cin), (3, Cin - 1)):
        assert lib.gct2_conv2d_s1_fwd(c.handle, F32, P, ld, P, None, P, Cout, B, H, W, Cin, Cout, ks, 1, None) == 1, ks
        assert lib.gct2_conv2d_s1_dgrad(c.handle, F32, P, Cout, P, None, 0, P, ld, B, H, W, Cin, Cout, ks, 0, None) == 1, ks
        assert lib.gct2_conv2d_s1_wgrad(c.handle, F32, P, ld, P, Cout, P, None, B, H, W, Cin, Cout, ks, 0, None) == 1, ks
    assert c.read_launch_log() == []
