"""The references of sdk_rows_fc (tests/rows_fc_ref.py) on a machine without a GPU: (a) every integer case of the GPU tests
(tests/test_rows_fc_paths_gpu.py) is exact in fp32 in any order and has no zero operand; (b) the float64 reference equals a second,
independent evaluation (exactly rounded sums of the expanded terms); (c) every row of the case table lands on the kernel it claims, by
the rule restated in Python and by sdk_rows_fc_path itself - so a change of the rule shows up here as well as on the GPU."""
import math

import numpy as np
import pytest

import rows_fc_ref as rf
from conftest import sub

LIB = sub("_lib")
BASE = 1 << 20                      # a 16-byte aligned "address": sdk_rows_fc_path looks at alignment only and never reads


@pytest.mark.parametrize("case", rf.INT_CASES, ids=rf.case_id)
def test_integer_cases_are_exact_in_any_order(case):
    for Nout in case.Nouts:
        x, s, t, w, bias = rf.int_operands(case.Cin, Nout)
        for a in (x, s, t, w, bias):
            assert a.dtype == np.float32 and np.all(a != 0) and np.array_equal(a, np.round(a))
        assert np.abs(x).max() <= 4 and np.abs(w).max() <= 4 and np.abs(s).max() <= 2 and np.all(np.abs(t) == 16) and np.abs(bias).max() <= 1024
        xp = x.astype(np.int64) * s.astype(np.int64) + t.astype(np.int64)
        assert np.all(xp != 0) and np.abs(xp).max() * np.abs(w).max() <= 96
        for _, aff, hb in rf.VARIANTS:
            tot = rf.abs_terms(x, s if aff else None, t if aff else None, w, bias if hb else None)
            assert tot.max() < 2 ** 24, (case, Nout, tot.max())
            for act in (0, 1):
                args = (x[:9], s if aff else None, t if aff else None, w, bias if hb else None, act)
                assert np.array_equal(rf.exact(*args).astype(np.float64), rf.f64(*args))       # the two references agree where both apply
            pre = rf.exact(x, s if aff else None, t if aff else None, w, bias if hb else None, 0)
            B = max(rf.B_PLAIN if (case.path_aff if aff else case.path_noaff) == 0 else rf.B_MFMA)
            assert Nout == 1 or ((pre[:B] < 0).any() and (pre[:B] > 0).any()), (case, Nout, B)   # the relu cuts some outputs and keeps others


def test_exact_reference_against_python_integers():
    x, s, t, w, bias = rf.int_operands(33, 5, 3)
    for aff in (True, False):
        for hb in (True, False):
            got = rf.exact(x, s if aff else None, t if aff else None, w, bias if hb else None, 0)
            for b in range(3):
                for j in range(5):
                    want = sum((int(x[b, c]) * int(s[c]) + int(t[c]) if aff else int(x[b, c])) * int(w[c, j]) for c in range(33)) + (int(bias[j]) if hb else 0)
                    assert int(got[b, j]) == want
                    assert int(rf.exact(x, s if aff else None, t if aff else None, w, bias if hb else None, 1)[b, j]) == max(want, 0)


@pytest.mark.parametrize("Cin,Nout", [(1, 1), (33, 7), (513, 33), (2176, 40)])
@pytest.mark.parametrize("act", [0, 1, 2])
def test_float64_reference_against_expanded_fsum(Cin, Nout, act):
    """second formulation: x' w expanded into x (s w) + t w, every product in float64, the sum exactly rounded (math.fsum)"""
    B = 3
    x, s, t, w, bias = rf.real_operands(Cin, Nout, B, act)
    for aff, hb in ((True, True), (False, True), (True, False)):
        got = rf.f64(x, s if aff else None, t if aff else None, w, bias if hb else None, act)
        tot = rf.abs_terms(x, s if aff else None, t if aff else None, w, bias if hb else None)
        if aff:                                                      # the expanded form's own terms: |x s w| + |t w| >= |x' w|
            tot = (np.abs(x.astype(np.float64) * s) + np.abs(t.astype(np.float64))) @ np.abs(w.astype(np.float64)) + (np.abs(bias) if hb else 0.0)
        bnd = rf.bound(x, s if aff else None, t if aff else None, w, bias if hb else None, act)
        for b in range(B):
            for j in range(0, Nout, max(1, Nout // 5)):
                if aff:
                    terms = [float(x[b, c]) * (float(s[c]) * float(w[c, j])) for c in range(Cin)] + [float(t[c]) * float(w[c, j]) for c in range(Cin)]
                else:
                    terms = [float(x[b, c]) * float(w[c, j]) for c in range(Cin)]
                v = math.fsum(terms + ([float(bias[j])] if hb else []))
                want = max(v, 0.0) if act == 1 else 1.0 / (1.0 + math.exp(-v)) if act == 2 else v
                assert abs(got[b, j] - want) <= (2 * Cin + 4) * 2.0 ** -53 * tot[b, j] + 4 * 2.0 ** -53, (b, j, got[b, j], want)
                assert bnd[b, j] > 1e6 * abs(got[b, j] - want)          # the reference's own error is nothing beside the fp32 bound
    if act == 2:
        v = rf.preact(x, s, t, w, bias)
        assert 19.0 <= np.abs(v[:min(4, B)]).max(1).min() and np.abs(v[:min(4, B)]).max() <= 21.0      # the scaled rows do sit near +-20


def _lib_path(lib, in_addr, ldin, aff, wt_addr, Cin, Nout):
    return lib.sdk_rows_fc_path(in_addr, ldin, int(aff), wt_addr, Cin, Nout)


def test_case_table_lands_on_the_claimed_paths():
    lib = LIB.load_library()
    seen = {}                                                       # path -> set of (has ring tail) over the integer cases
    for c in rf.INT_CASES:
        for Nout in c.Nouts:
            in_off, ldin, wt_off = rf.case_layout(c, Nout)
            for _, aff, _ in rf.VARIANTS:
                want = c.path_aff if aff else c.path_noaff
                assert rf.path(BASE + in_off, ldin, aff, BASE + wt_off, c.Cin, Nout) == want, (c, Nout, aff)
                assert _lib_path(lib, BASE + in_off, ldin, aff, BASE + wt_off, c.Cin, Nout) == want, (c, Nout, aff)
                # a row slice of a batch (row r at byte offset 4 r ldin) stays on the path: what the row-independence test relies on
                for r in (1, 2, 3, 64):
                    assert rf.path(BASE + in_off + 4 * r * ldin, ldin, aff, BASE + wt_off, c.Cin, Nout) == want
                seen.setdefault(want, set()).add(want != 0 and rf.ring(want, c.Cin)[2] > 0)
    assert seen == {0: {False}, 1: {False, True}, 2: {False, True}, 3: {False, True}}, seen
    for p, Cin, Nout in rf.STRIDED_CASES:
        for aff in (True, False):
            assert rf.path(BASE, Cin + 8, aff, BASE, Cin, Nout) == p == _lib_path(lib, BASE, Cin + 8, aff, BASE, Cin, Nout)
        assert p == 0 or rf.ring(p, Cin)[2] > 0
    for p, Cin, Nout in rf.REAL_CASES:
        for aff in (True, False):
            assert rf.path(BASE, Cin, aff, BASE, Cin, Nout) == p == _lib_path(lib, BASE, Cin, aff, BASE, Cin, Nout)
    for p in (1, 2, 3):                                             # one steady-state and one tail shape per matrix-pipe path
        assert {rf.ring(p, Cin)[2] > 0 for q, Cin, _ in rf.REAL_CASES if q == p} == {False, True}
    # the ring regimes the issue names: start-up (ng < D), full turns + tail, no tail
    assert [rf.ring(1, c) for c in (32, 96, 128, 160, 224, 2016, 2080)] == [(1, 0, 1), (3, 0, 3), (4, 1, 0), (5, 1, 1), (7, 1, 3), (63, 15, 3), (65, 16, 1)]
    assert [rf.ring(2, c) for c in (2048, 2176, 2432, 8320)] == [(16, 4, 0), (17, 4, 1), (19, 4, 3), (65, 16, 1)]
    assert [rf.ring(3, c) for c in (2048, 2176, 2944, 8192)] == [(16, 2, 0), (17, 2, 1), (23, 2, 7), (64, 8, 0)]


def test_rule_and_library_agree_on_a_grid_of_shapes_and_alignments():
    lib = LIB.load_library()
    for Cin in (1, 31, 32, 33, 64, 127, 128, 2016, 2047, 2048, 2080, 2176, 8192, 8320, 16384):
        for Nout in (1, 31, 32, 33, 64, 192):
            for in_off in (0, 4, 8, 16):
                for wt_off in (0, 4, 16):
                    for ldin in (Cin, Cin + 1, Cin + 2, Cin + 4):
                        for aff in (0, 1):
                            args = (BASE + in_off, ldin, aff, BASE + wt_off, Cin, Nout)
                            assert _lib_path(lib, *args) == rf.path(*args), args
    # the limits themselves
    assert _lib_path(lib, BASE, 8192, 1, BASE, 8192, 32) == 3 and _lib_path(lib, BASE, 8320, 1, BASE, 8320, 32) == 0
    assert _lib_path(lib, BASE, 8320, 0, BASE, 8320, 32) == 3
    assert _lib_path(lib, BASE, 1920, 0, BASE, 1920, 32) == 1 and _lib_path(lib, BASE, 2048, 0, BASE, 2048, 32) == 3
    # the shapes the models use: ECAPA's final FC and context bias, the SE heads, x-vector (3000) and ResNet34 (5120)
    for Cin, Nout, aff, want in ((6144, 192, 1, 3), (6144, 128, 0, 3), (1024, 128, 0, 1), (128, 1024, 0, 1), (3000, 512, 0, 0), (5120, 256, 0, 3)):
        assert _lib_path(lib, BASE, Cin, aff, BASE, Cin, Nout) == want, (Cin, Nout)
