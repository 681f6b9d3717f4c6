"""The geometry of tests/large_view_cases.py, checked without a GPU: every case's images sit on the intended sides of its boundary,
T0 / T0+ straddle the restated predicates, the exact-sum budgets hold at the cases' shapes, no case needs more than 10 GiB of device
memory, and exactly one operand per case is large."""
import numpy as np
import pytest
import torch

import exact_cases as E
import large_view_cases as L
from exact_cases import BF16, F16, F32

CASES = L.all_cases()
IDS = [c.id for c in CASES]


def test_case_ids_are_unique_and_the_lists_are_not_empty():
    assert len(set(IDS)) == len(IDS), sorted(i for i in IDS if IDS.count(i) > 1)
    for f in (L.layer_cases, L.plane_cases, L.colsum_cases, L.many_pixel_cases, L.head_cases, L.pointwise_cases, L.dense_head_cases):
        assert f()


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_images_sit_on_the_intended_sides(c):
    B, h, w, C = c.view
    assert 3 <= B <= 5 and B == c.shape[0] == (L.MANY_SHAPE[0] if c.kind == "many" else L.TIER_GEOMETRY[c.tier][0])
    assert c.ld >= C and c.span == ((B * h * w - 1) * c.ld + C) * c.es
    if c.tier in ("T0", "T0+"):
        return
    bound = L.TIER_BYTES[c.tier]
    below, above = L.sides(c.tier, B, h * w, c.ld, C, c.es)
    assert c.span > bound and below and below[0] == 0
    if c.tier == "T3":
        # the last image straddles 2^33 (a whole image above it does not fit into 10 GiB: large_view_cases.py): four whole images
        # below, and of image 4 at least one whole row below and - where it has more than two rows - at least a third of them above
        assert below == [0, 1, 2, 3] and above == []
        rb, ra = L.last_image_rows(c.tier, B, h, w, c.ld, C, c.es)
        if h > 2:
            assert rb >= 1 and ra >= h // 3, (rb, ra, h)
        else:
            lo, hi = L.image_range(B - 1, h * w, c.ld, C, c.es)
            assert lo < bound < hi - c.ld * c.es          # ... else at least its last pixel
    else:
        assert above and above[-1] == B - 1, (below, above)
    # "just over": the next smaller stride would put the boundary behind the tier's position
    if c.kind != "many":
        f = L.TIER_GEOMETRY[c.tier][1]
        step = c.ld - L.tier_ld(c.tier, h * w, C, c.es, 1)
        assert 0 <= step < 8 and f * h * w * c.ld * c.es >= bound


@pytest.mark.parametrize("c", [c for c in CASES if c.tier in ("T0", "T0+")], ids=lambda c: c.id)
def test_t0_and_t0_plus_straddle_the_restated_predicate(c):
    assert c.ld % 8 == 0
    if c.tier == "T0":
        assert c.predicate(c.ld) and not c.predicate(c.ld + 8)
        assert (c.family or "").startswith(("tap:", "halo:", "wgrad:"))          # the matrix-core family
    else:
        assert c.predicate(c.ld - 8) and not c.predicate(c.ld)
        assert not (c.family or "").startswith(("tap:", "halo:", "wgrad:"))
    # the operand is large in earnest: a fifth of the limit and more (the transposed and stride-1 forms count their source four times)
    assert c.span * (4 if c.kind != "head" and c.entry in ("convT_fwd", "conv_dgrad", "s1_fwd", "s1_dgrad") else 1) > 0.2 * L.LIMIT


def test_predicates_at_the_values_the_library_comments_give():
    """spot values computed by hand from the comments in csrc/ (a restatement that drifted would fail here)"""
    # tapgemm: B = 1, 2 x 2 small grid, K = N = 8: 16 ld * 2 + 5 ld * 2 + 15 ld * 2 + 16 = 72 ld + 16 < 0x7ff00000
    assert L.tapgemm_admits(1, 2, 2, 8, 8, (0x7ff00000 - 17) // 72) and not L.tapgemm_admits(1, 2, 2, 8, 8, (0x7ff00000 - 17) // 72 + 1)
    # wgrad: 4 pixels, big on the doubled grid: 16 ld * 2
    assert L.wgrad_admits(1, 2, 2, 0, 0x7ff00000 // 32 - 1, 8) and not L.wgrad_admits(1, 2, 2, 0, 0x7ff00000 // 32, 8)
    assert L.wgrad_admits(1, 2, 2, 3, 0x7ff00000 // 8 - 1, 8) and not L.wgrad_admits(1, 2, 2, 3, 8, 0x7ff00000 // 8)
    # head: 256 pixels: 512 ld + 128 + 16
    assert L.head_admits(1, 16, 16, 8, 64, 0x7ff00000 // 512 - 8) and not L.head_admits(1, 16, 16, 8, 64, 0x7ff00000 // 512)
    assert not L.head_admits(1, 16, 16, 0x7ff00000 // 2048, 64, 8)               # the kernel tensor: 16 * K * 64 * 2


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_no_case_needs_more_than_10_gib_and_one_operand_is_large(c):
    total = L.device_bytes(c)
    assert total <= L.MAX_DEVICE_BYTES, (total / 2 ** 30)
    assert total - c.span - 2 * c.view[2] * c.ld * c.es <= 1 << 30               # everything but the wide buffer is compact
    assert c.span >= 0.2 * L.LIMIT
    assert c.ld < 1 << 31                                                        # `ld` is an int of the C interface


LAYER = [c for c in CASES if c.kind in ("tap", "s1", "wgrad", "colsum", "plane", "many")]


@pytest.mark.parametrize("key", sorted({(c.entry, c.shape, c.dt, c.special) for c in LAYER}, key=repr), ids=repr)
def test_exact_sum_budget_of_the_layer_inputs(key):
    """the inputs of the large cases are exact_cases.make_case's at shapes tests/test_exact_cases_cpu.py does not list"""
    entry, shape, dt, special = key
    cs = E.make_case(entry, shape, dt, special)
    E.assert_budget(cs.ops)
    for name in ("x", "dz", "w", "act", "prev"):
        if hasattr(cs, name):
            storage = F32 if name == "bias" else dt
            assert E.survives_storage(getattr(cs, name), storage), name
    E.expected(cs.ref, cs.out_dt)              # (asserts that the reference is exact in float32)


@pytest.mark.parametrize("key", sorted({(c.shape[:4], c.dt) for c in L.head_cases()}, key=repr), ids=repr)
def test_exact_sum_budget_of_the_head_inputs(key):
    shape, dt = key
    cs = E.make_case("convT_head", shape, dt)
    E.assert_budget(cs.ops)
    assert E.survives_storage(cs.xc, dt) and E.survives_storage(cs.wc, dt) and E.survives_storage(cs.bc, F32) and E.survives_storage(cs.x, dt)
    assert E.survives_storage(cs.w, F32) and E.survives_storage(cs.bias, F32) and E.survives_storage(cs.target, F32)
    for name, magnitude, step in E.head_budgets(cs, cs.x):
        assert magnitude / step < E.BUDGET, (name, magnitude / step)
    assert np.array_equal(cs.d, cs.delta * cs.lsb) and float((cs.delta ** 2).sum()) < 2.0 ** 24
    for r in (cs.y, cs.pred, cs.pred_r, cs.d, cs.dpred, cs.dx, cs.dw, cs.db, cs.db_dx):
        E.expected(r, F32)


def test_dense_head_train_ldx_limit_is_the_restated_one():
    fits = lambda ldx: 256 * ldx * 2 + 256 * 64 * 2 + 256 * 16 + ldx * 16 <= 160 * 1024
    assert fits(L.DENSE_HEAD_LDX_MAX) and not fits(L.DENSE_HEAD_LDX_MAX + 8)
    assert 2 ** 31 // (L.DENSE_HEAD_LDX_MAX * 2) > 100 * max(E.HEAD_MS)         # pixels of a 2-GiB view at that stride


@pytest.mark.parametrize("dt", [F32, BF16, F16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("B", sorted({c.view[0] for c in L.pointwise_cases() if c.entry.startswith("dense_")}))
def test_exact_sum_budget_of_the_dense_inputs(B, dt):
    """M = B * 250 rows: exact_cases._dense_case asserts its own budgets when it builds the case"""
    h, w = L.DENSE_HW
    cs = E.make_case("dense_fwd", (B * h * w, 67, 3), dt)
    E.assert_budget(cs.ops)
    for r in (cs.pred, cs.dx, cs.dw, cs.db):
        E.expected(r, F32)


@pytest.mark.parametrize("tdt", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
def test_wide_view_and_its_untouched_check_on_the_host(tdt):
    """exact_cases.wide_view / assert_outside_untouched_device at a small stride, on CPU tensors: the view holds the tensor at the
    stated stride behind one guard row, a write inside the view passes, a write anywhere else - a pad channel, a guard row - fails"""
    t = torch.arange(2 * 3 * 4 * 5, dtype=torch.float32).reshape(2, 3, 4, 5).to(tdt)
    ld = 11
    for fill in (float("nan"), E.SENTINEL):
        buf, view, ptr = E.wide_view(t, ld, fill)
        assert buf.numel() == 4 * ld + (2 * 3 * 4 - 1) * ld + 5 + 4 * ld and ptr == buf.data_ptr() + 4 * ld * buf.element_size()
        assert torch.equal(view, t) and torch.equal(buf[4 * ld + 7 * ld:][:5], t.reshape(-1, 5)[7])
        view[1, 2, 3, 4] = 7.0
        E.assert_outside_untouched_device(buf, view, fill)
        assert bool((buf.view(torch.int32 if tdt == torch.float32 else torch.int16) == buf.view(torch.int32 if tdt == torch.float32 else torch.int16)[0]).all())      # (masked: the whole buffer is fill again)
        for where in (4 * ld + 5, 0, buf.numel() - 1, 4 * ld - 1):
            buf2, view2, _ = E.wide_view(t, ld, fill)
            buf2[where] = 3.0
            with pytest.raises(AssertionError, match=f"first at element {where} "):
                E.assert_outside_untouched_device(buf2, view2, fill)


def test_engine_predicate_is_the_restated_head_bound():
    """UNetEngine.fused_u0_head_ok's size term (engine.u0_head_sizes_ok) against large_view_cases.head_admits, around the bound of
    the source and of the kernel"""
    from gan_class_transfer2_amd import engine
    assert engine.U0_HEAD_MAX_BYTES == L.LIMIT
    for B, H, W, K in ((4, 16, 16, 16), (1, 16, 16, 8), (64, 64, 64, 128)):
        top = L.largest_ld(lambda ld: L.head_admits(B, H, W, K, 64, ld), K)
        for ld in (K, top - 8, top, top + 8, 2 * top):
            assert engine.u0_head_sizes_ok(B, H, W, ld, K, 64) == L.head_admits(B, H, W, K, 64, ld) == (ld <= top), (B, H, W, K, ld)
    k_top = L.LIMIT // 2048
    assert engine.u0_head_sizes_ok(1, 16, 16, k_top - 8, k_top - 8, 64) and not engine.u0_head_sizes_ok(1, 16, 16, k_top, k_top, 64)


@pytest.mark.parametrize("key", sorted({(c.view[0] * c.view[1] * c.view[2], c.dt) for c in L.dense_head_cases()}), ids=repr)
def test_exact_sum_budget_of_the_dense_head_inputs(key):
    """gct2_dense_head_train at M = B * 250: M = 1000 is tests/exact_cases.py's own, M = 1250 takes the ranges of its larger sizes"""
    M, dt = key
    cs = E.make_case("head_train", (M, 67, 3), dt)
    assert E.survives_storage(cs.x, dt) and E.survives_storage(cs.w, F32) and E.survives_storage(cs.bias, F32) and E.survives_storage(cs.target, F32)
    for name, magnitude, step in E.head_budgets(cs, cs.x):
        assert magnitude / step < E.BUDGET, (name, magnitude / step)
    assert np.array_equal(cs.d, cs.delta * cs.lsb) and float((cs.delta ** 2).sum()) < 2.0 ** 24
    for r in (cs.pred, cs.pred_r, cs.d, cs.dpred, cs.dx, cs.dw, cs.db, cs.db_dx, cs.db_dx_stored):
        E.expected(r, F32)


def test_every_role_of_every_layer_entry_has_the_tiers_of_the_table():
    """16-bit: sources at T0, T0+, T1, T2, T3, other roles at T1 .. T3; fp32 direct and fp32 matrix cores: every role at T2 and T3.
    Pointwise: every view at T1, T2 and T3; and every operand of the file has a case at T2 or above"""
    have = {}
    for c in L.layer_cases():
        if c.shape[1:] == L.LAYER_ENTRIES[c.entry][1][1:] and c.tuning == (L.LAYER_ENTRIES[c.entry][2] if c.dt != F32 else 0):
            have.setdefault((c.entry, c.role, "16" if c.dt != F32 else c.mode), set()).add(c.tier)
    for entry, (kind, shape, *_rest) in L.LAYER_ENTRIES.items():
        for role in L.operands(entry, shape):
            want16 = {"T1", "T2", "T3"} | ({"T0", "T0+"} if L.is_source(entry, role) else set())
            assert have[(entry, role, "16")] == want16, (entry, role, have.get((entry, role, "16")))
            assert have[(entry, role, "f32")] == have[(entry, role, "f32m")] == {"T2", "T3"}, (entry, role)
    pw = {}
    for c in L.pointwise_cases():
        pw.setdefault((c.entry, c.role), set()).add(c.tier)
    assert len(pw) == sum(len(roles) for _e, roles, _m in L.POINTWISE) and all(t == {"T1", "T2", "T3"} for t in pw.values()), pw
