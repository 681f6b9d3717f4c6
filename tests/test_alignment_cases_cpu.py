"""tests/alignment_cases.py checked without a GPU: every placement of the case table produces the residues it states, holds the tensor
and the fill everywhere else; the restated predicates send every case to the family and branch the table names; every branch of
DESIGN.md's "Alignment classes" table is reached; and every case runs on inputs that tests/test_exact_cases_cpu.py has vetted."""
import numpy as np
import pytest
import torch

import alignment_cases as A
import exact_cases as E
from exact_cases import BF16, F16, F32, SENTINEL
from test_kernels_exact_gpu import MODE_DT

CASES = A.CASES
IDS = [A.case_id(c) for c in CASES]


def place_all(c):
    """every operand of the case through its placement, on the host: role -> (buffer or output object, pointer, ld, tensor)"""
    place = A.Aligned(c.placement)
    made = {}
    for role, shape in A.role_shapes(c.entry, c.shape).items():
        n = int(np.prod(shape))
        t = (torch.arange(n, dtype=torch.float32) % 251 + 1).reshape(shape).to(A.role_dtype(role, c.mode))
        if role in ("y", "dx"):
            o, ld = place.out(role, t, c.mode)
            made[role] = (o, o.ptr, ld, t)
        elif role in ("dw", "db", "db2"):
            o = place.grad(role, t)
            made[role] = (o, o.ptr, 0, t)
        elif role in ("w", "bias"):
            buf, ptr = place.param(role, t)
            made[role] = (buf, ptr, 0, t)
        else:
            buf, ptr, ld = place.inp(role, t, c.mode, "act" if role == "act" else "in")
            made[role] = (buf, ptr, ld, t)
    return place, made


def test_ids_are_unique_and_every_group_is_there():
    assert len(set(IDS)) == len(IDS)
    assert {c.group for c in CASES} == set("abcdefghi")
    for c in CASES:
        assert c.mode in MODE_DT and set(c.placement) <= set(A.role_shapes(c.entry, c.shape))


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_placement_gives_its_residues_and_holds_the_tensor(c):
    place, made = place_all(c)
    for role, (obj, ptr, ld, t) in made.items():
        want = place.of(role)
        es = t.element_size()
        buf = obj if isinstance(obj, torch.Tensor) else obj.buf
        assert buf.data_ptr() % 64 == 0 and place.seen[role] == (ptr, ld)
        fill = torch.tensor(A.FILL[role], dtype=t.dtype)          # (bf16 stores the sentinel rounded: compare with the stored value)
        flat = buf.reshape(-1)
        start = (ptr - buf.data_ptr()) // es
        assert (ptr - buf.data_ptr()) % es == 0
        if role in A.VIEW_ROLES:
            ptr_res, ld_res = want
            assert ptr % 16 == ptr_res and (ld == ld_res[1] if isinstance(ld_res, tuple) else ld % 8 == ld_res) and ld >= t.shape[-1]
            npix = t.numel() // t.shape[-1]
            idx = (torch.arange(npix)[:, None] * ld + torch.arange(t.shape[-1])[None, :] + start).reshape(-1)
        else:
            assert ptr % 16 == want
            idx = torch.arange(t.numel()) + start
        assert torch.equal(flat[idx], t.reshape(-1))
        rest = torch.ones(flat.numel(), dtype=torch.bool)
        rest[idx] = False
        other = flat[rest]
        assert bool(torch.isnan(other).all()) if np.isnan(A.FILL[role]) else bool((other == fill).all())
        # guards on both sides: a row of pixels (views) / E.GUARD elements (arrays)
        assert start >= E.GUARD and flat.numel() - int(idx.max()) - 1 >= E.GUARD


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_predicates_send_the_case_where_the_table_says(c):
    place, made = place_all(c)
    got = A.predict(c.entry, c.shape, c.mode, place.seen, c.tuning, c.workspace, split=c.opts.get("split", False))
    assert got == (c.family, c.branch), got
    if c.opts.get("way") == "act8":                 # without the mask the same call takes the 16-byte side
        wide = A.predict(c.entry, c.shape, c.mode, place.seen, c.tuning, c.workspace, masked=False)
        assert wide == (("halo:convT:", "halo") if c.group == "e" else (c.family, "e16")), wide


def test_aligned_placement_takes_the_aligned_side_everywhere():
    """the other side of every choice: the same predicates on the all-aligned placement name the 16-byte paths"""
    seen = set()
    for c in CASES:
        key = (c.entry, c.shape, c.mode, c.tuning, c.workspace)
        if key in seen:
            continue
        seen.add(key)
        place, _ = place_all(c._replace(placement={}))
        family, branch = A.predict(c.entry, c.shape, c.mode, place.seen, c.tuning, c.workspace, split=c.opts.get("split", False))
        if c.mode.startswith("f32m"):
            assert branch.startswith("avec1:bvec1")
        elif c.entry == "conv_fwd" and c.shape[3] <= 4:
            assert (family, branch.split(":")[0]) == ("rgb:fwd", "vec8") and "plain" not in branch
        elif c.entry == "conv_wgrad" and c.shape[3] <= 4:
            assert (family, branch) == ("rgb:wgrad", "vec8:slabs-allowed" if c.workspace else "vec8:no-slabs")
        elif c.entry.endswith("_wgrad"):
            assert family in ("wgrad:", "wgrad:s1:")
        elif c.group == "e":
            assert family == "halo:convT:"
        else:
            assert family.startswith("tap:") and branch in ("e16", "finalize")


def test_every_branch_of_the_design_table_is_reached():
    for name, (family, prefix) in A.BRANCHES.items():
        hits = [c for c in CASES if (c.family == family if family is None or c.family is None else c.family.startswith(family))
                and c.branch.startswith(prefix)]
        assert hits, name
    text = open(__file__.rsplit("/tests/", 1)[0] + "/DESIGN.md").read()
    assert "Alignment classes" in text
    for c in CASES:            # and the table names nothing but branches the predicates can return
        assert c.branch.split(":")[0] in ("e8", "finalize8", "direct", "vec8", "scalar", "avec0", "avec1"), c.branch


def used_inputs():
    return sorted({(c.entry, c.shape, MODE_DT[c.mode], A.case_special(c)) for c in CASES}, key=str)


def test_inputs_are_the_vetted_ones():
    """no case brings inputs of its own: each one is a case of tests/test_exact_cases_cpu.py's quality checks"""
    vetted = set(E.reference_cases()) | set(E.special_cases())
    for case in used_inputs():
        assert case in vetted, case


@pytest.mark.parametrize("case", used_inputs(), ids=lambda k: f"{k[0]}-{'x'.join(map(str, k[1]))}-{E.DTYPE_NAMES[k[2]]}-{k[3]}")
def test_inputs_keep_the_budget(case):
    E.assert_budget(E.make_case(*case).ops)


def test_guarded_offset_keeps_both_guards():
    t = torch.arange(10, dtype=torch.float32)
    for off in (0, 1, 2, 3):
        buf, ptr = E.guarded(t, SENTINEL, off)
        assert ptr == buf.data_ptr() + 4 * (E.GUARD + off) and buf.numel() == 10 + 2 * E.GUARD + off
        assert torch.equal(buf[E.GUARD + off:E.GUARD + off + 10], t)
        assert bool((buf[:E.GUARD + off] == SENTINEL).all()) and bool((buf[-E.GUARD:] == SENTINEL).all())
    assert torch.equal(E.guarded_data(E.guarded(t)[0], (10,)), t)


def test_flat_out_sees_a_write_beside_the_view():
    t = torch.zeros(1, 2, 3, 5, dtype=torch.float16)
    o = A.FlatOut(t, 12, 8)
    assert o.ptr % 16 == 8
    o.view.fill_(3.0)
    o.check(torch.full_like(t, 3.0), "inside")
    start = (o.ptr - o.buf.data_ptr()) // 2
    for at in (start - 1, start + 5, start + 12 * 5 + 5, 0, o.buf.numel() - 1):
        keep = o.buf[at].clone()
        o.buf[at] = 1.0
        with pytest.raises(AssertionError, match="outside the view"):
            o.check(torch.full_like(t, 3.0), "beside")
        o.buf[at] = keep
    o.check(torch.full_like(t, 3.0), "restored")
