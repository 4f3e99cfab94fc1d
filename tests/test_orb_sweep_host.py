"""The OrbDetector sweep on the CPU: on every case of orb_cases.py the oracle's detector equals the restatement bit for bit, and the
restatement's own counts meet the premises the case was made for (which select cuts, where the cut falls, how many levels run).
This is what shows, with the reference alone, that the inputs of test_orb_sweep_gpu.py reach what they are meant to reach."""
import numpy as np
import pytest

import orb_cases as oc
from golden import make_golden as mg


@pytest.mark.parametrize("name", sorted(oc.FAMILIES))
def test_oracle_equals_the_restatement_and_the_premises_hold(oracle, name):
    fast = oc.oracle_fast(oracle)
    cases = oc.family(name, fast)
    assert cases
    for case in cases:
        ref, levels = oc.reference(case, fast)
        print("%r: %d keypoints, %d rejected; %s" % (case, len(ref), case.rejected, oc.describe(levels)))
        assert case.premise is not None or name == "d", case
        if case.premise is not None:
            case.premise(levels)
        assert oc.same_level_sizes(case), case
        got = oc.detect(oracle, case)
        assert oc.same_rows(got, ref), (case, got.shape, ref.shape)
        assert len(ref) == sum(L["n2"] for L in levels) and np.array_equal(ref[:, 5], np.sort(ref[:, 5]))       # level by level, lowest first


def test_case_list_is_complete(oracle):
    """Every family of the issue is there with the parameters it names, and the list is the same on a second build."""
    fast = oc.oracle_fast(oracle)
    cases = oc.all_cases(fast)
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    assert [sum(1 for c in cases if c.family == f) for f in "abcdefg"] == [5, 2, 2, 13, 16, 2, 2]
    assert all(max(c.img.shape) <= 500 and min(c.img.shape) <= 300 for c in cases)
    d = [c for c in cases if c.family == "d"]
    assert sorted(set((c.patch, c.edge) for c in d)) == sorted(oc.PATCH_EDGE) and all(c.nlevels == 3 for c in d)
    assert set(c.img.shape for c in d) == {oc.SMALL, oc.LARGE, (16, 16)}
    e = [c for c in cases if c.family == "e"]
    assert set(c.scale_factor for c in e) == {1.2, 1.5, 2.0, 1.05} and set(c.nlevels for c in e) >= {1, 2, 8, 16}
    assert set(c.nfeatures for c in e if c.nlevels == 8 and c.scale_factor == 1.2) == {0, 1, 2, 7, 60, 1500, 100000}
    f = [c for c in cases if c.family == "f"]
    assert all(c.strided for c in f) and set(c.name[len("f_strided_"):][0] for c in f) == {"a", "e"}
    assert all(c.python_fast and c.nlevels == 2 for c in cases if c.family == "g") and not any(c.python_fast for c in cases if c.family != "g")
    rebuilt = [c for n in sorted(oc.FAMILIES) for c in oc.FAMILIES[n](fast)]
    assert [repr(c) for c in rebuilt] == [repr(c) for c in cases] and all(a.img is b.img for a, b in zip(rebuilt, cases))


def test_strided_view_is_the_trackers_region_call(oracle):
    img = oc.block_image(*oc.SMALL)
    view = oc.strided_view(img)
    assert view.strides == (img.shape[1] + 5, 1) and np.array_equal(view, img)
    buf = view
    while buf.base is not None:
        buf = buf.base
    assert view.ctypes.data - buf.ctypes.data == 3
    mask = np.ones(len(buf), bool)
    mask[3:].reshape(img.shape[0], -1)[:, :img.shape[1]] = False
    assert (buf[mask] == 255).all() and mask.sum() == 3 + 5 * img.shape[0]
    with pytest.raises(ValueError):
        oracle.orb_detect(view, 50, 1.2, 2, 8, 15, 20, row_stride=img.shape[1])         # not the view's own stride
    with pytest.raises(ValueError):
        oracle.orb_detect(view.astype(np.int16), 50, 1.2, 2, 8, 15, 20, row_stride=view.strides[0])
    dense = oracle.orb_detect(img, 50, 1.2, 2, 8, 15, 20)
    assert len(dense) and oc.same_rows(oracle.orb_detect(view, 50, 1.2, 2, 8, 15, 20, row_stride=view.strides[0]), dense)
    assert oc.same_rows(oracle.orb_detect(view, 50, 1.2, 2, 8, 15, 20), dense)          # the default still takes a dense copy


def test_restatement_with_the_python_fast_is_make_goldens(golden):
    """With its default FAST the restatement is make_golden.orb_detect_ref on the committed fixture's image: the joins restated in
    orb_cases.py (quotas, pyramid, selects, scale-back) against the ones the fixture was made with."""
    img = golden["orb"]["img"][:100, :130]
    got, levels = oc.orb_detect_ref(img, 24, 1.2, 2, 31, 31, 20)
    assert oc.same_rows(got, mg.orb_detect_ref(img, 24, 1.2, 2, 31, 31, 20)) and len(got) and len(levels) == 2
