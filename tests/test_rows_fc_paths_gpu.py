"""sdk_rows_fc (csrc/pool_se.hip) on each of its four kernels, against the references of tests/rows_fc_ref.py.  Every case first asserts
that sdk_rows_fc_path puts its arguments on the intended kernel (0 plain, 1 rows_fc_mfma_kernel<4>, 2 <16, false>, 3 <16, true>), then
judges the result: integer operands bit for bit against int64 (any dropped, duplicated or misplaced term shows), real operands against
float64 by the bound n 2^-24 sum|terms|.  Shapes walk the register ring of the matrix-pipe kernels through start-up (ng < D), full turns and
every tail, and the 32-row / 4-row block edges; outputs land in sentinel-filled buffers and nothing outside [B, Nout] may change."""
import numpy as np
import pytest
import torch

import rows_fc_ref as rf
from conftest import sub

pytestmark = pytest.mark.gpu

L = sub("_lib")
SENT = -7.75                         # sentinel around every output
POISON = 1000.0                      # padding of `in` rows and around `wt`: a read outside [B, Cin] x [Cin, Nout] breaks the integer result


def _s():
    return torch.cuda.current_stream().cuda_stream


class Operands:
    """device copies of (x, s, t, w, bias) in a given layout: `in` in_off bytes into its buffer with row stride ldin, `wt` wt_off bytes in"""

    def __init__(self, x, s, t, w, bias, in_off=0, ldin=None, wt_off=0):
        B, Cin = x.shape
        ldin = ldin or Cin
        xb = torch.full((in_off // 4 + B * ldin + 4,), POISON, dtype=torch.float32)
        xv = xb[in_off // 4: in_off // 4 + B * ldin].view(B, ldin)
        xv[:, :Cin] = torch.from_numpy(x)
        self.xbuf = xb.cuda()
        self.x = self.xbuf[in_off // 4: in_off // 4 + B * ldin].view(B, ldin)[:, :Cin]
        wb = torch.full((wt_off // 4 + w.size + 4,), POISON, dtype=torch.float32)
        wb[wt_off // 4: wt_off // 4 + w.size] = torch.from_numpy(w).reshape(-1)
        self.wbuf = wb.cuda()
        self.w = self.wbuf[wt_off // 4: wt_off // 4 + w.size].view(*w.shape)
        self.s, self.t, self.bias = (torch.from_numpy(a).cuda() for a in (s, t, bias))
        self.Cin, self.Nout, self.ldin = Cin, w.shape[1], ldin
        assert self.x.data_ptr() % 16 == in_off % 16 and self.w.data_ptr() % 16 == wt_off % 16 and self.x.stride(0) == ldin


def _raw(eng, x_ptr, ldin, s, t, w_ptr, bias, out, B, Cin, Nout, act):
    return eng.lib.sdk_rows_fc(eng.ctx, x_ptr, ldin, s.data_ptr() if s is not None else None, t.data_ptr() if t is not None else None, w_ptr,
                               bias.data_ptr() if bias is not None else None, out.data_ptr(), out.stride(0), B, Cin, Nout, act, _s())


def _run(eng, ops, B, act, aff, hb, want_path, ld_extra=0, row0=0):
    """rows row0 .. row0 + B of the operands through sdk_rows_fc into a sentinel-filled [B + 3, Nout + ld_extra] buffer; asserts the path
    and that nothing outside [B, Nout] changed; returns the output as float64 numpy"""
    x_ptr = ops.x.data_ptr() + 4 * row0 * ops.ldin
    got_path = eng.lib.sdk_rows_fc_path(x_ptr, ops.ldin, int(aff), ops.w.data_ptr(), ops.Cin, ops.Nout)
    assert got_path == want_path, f"Cin {ops.Cin} Nout {ops.Nout} affine {aff}: path {got_path}, the case is meant for path {want_path}"
    buf = torch.full((B + 3, ops.Nout + ld_extra), SENT, dtype=torch.float32, device="cuda")
    L.check(_raw(eng, x_ptr, ops.ldin, ops.s if aff else None, ops.t if aff else None, ops.w.data_ptr(), ops.bias if hb else None,
                 buf, B, ops.Cin, ops.Nout, act), "sdk_rows_fc")
    torch.cuda.synchronize()
    b = buf.cpu().numpy()
    assert (b[B:] == SENT).all() and (b[:, ops.Nout:] == SENT).all(), f"store outside the output (B {B} Nout {ops.Nout} ld_extra {ld_extra})"
    return b[:B, :ops.Nout].astype(np.float64)


def _int_check(eng, x, s, t, w, bias, ops, Bs_of_path, paths, ld_extra, what):
    for name, aff, hb in rf.VARIANTS:
        p = paths[0] if aff else paths[1]
        core = rf.exact(x, s if aff else None, t if aff else None, w, None, 0)             # int64; the bias and the relu follow
        for act in (0, 1):
            want = core + (bias.astype(np.int64) if hb else 0)
            want = (np.maximum(want, 0) if act == 1 else want).astype(np.float64)
            for B in Bs_of_path[p]:
                got = _run(eng, ops, B, act, aff, hb, p, ld_extra)
                bad = got != want[:B]
                assert not bad.any(), (f"{what} {name} act {act} B {B} path {p}: {int(bad.sum())} / {bad.size} outputs differ from the exact integer "
                                       f"result, first at {tuple(np.argwhere(bad)[0])}: got {got[bad][0]}, want {want[:B][bad][0]}")


BS = {0: rf.B_PLAIN, 1: rf.B_MFMA, 2: rf.B_MFMA, 3: rf.B_MFMA}


@pytest.mark.parametrize("case", rf.INT_CASES, ids=rf.case_id)
def test_integer_operands_are_exact_on_every_path(engine, case):
    """the case table of tests/rows_fc_ref.py: with affine and bias, without the affine, without the bias; act 0 and 1; every B on the block edges"""
    for Nout in case.Nouts:
        x, s, t, w, bias = rf.int_operands(case.Cin, Nout)
        in_off, ldin, wt_off = rf.case_layout(case, Nout)
        ops = Operands(x, s, t, w, bias, in_off, ldin, wt_off)
        _int_check(engine, x, s, t, w, bias, ops, BS, (case.path_aff, case.path_noaff), 0, f"Cin {case.Cin} Nout {Nout} {case.layout}")


@pytest.mark.parametrize("p,Cin,Nout", rf.STRIDED_CASES)
def test_integer_operands_with_row_strides(engine, p, Cin, Nout):
    """ldin = Cin + 8 (poisoned padding) and ldout = Nout + 24 (sentinel padding) on every path"""
    x, s, t, w, bias = rf.int_operands(Cin, Nout)
    ops = Operands(x, s, t, w, bias, 0, Cin + 8, 0)
    _int_check(engine, x, s, t, w, bias, ops, BS, (p, p), 24, f"strided Cin {Cin} Nout {Nout}")


def _judge(got, want, bound, what):
    err = np.abs(got - want)
    ratio = float((err / np.maximum(bound, 1e-300)).max())
    bad = ~(err <= bound)
    assert not bad.any(), f"{what}: {int(bad.sum())} / {bad.size} outside the bound, worst err / bound {ratio:.3g}"
    print(f"{what}: worst err / bound {ratio:.3g}")
    return ratio


@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("p,Cin,Nout", rf.REAL_CASES)
def test_real_operands_within_the_fp32_bound(engine, p, Cin, Nout, act):
    """x ~ N(0, 1), w ~ N(0, 1) / sqrt(Cin) against float64; act = 2 with four rows scaled to pre-activations near +-20"""
    B = 9 if p == 0 else 65
    x, s, t, w, bias = rf.real_operands(Cin, Nout, B, act)
    ops = Operands(x, s, t, w, bias)
    for name, aff, hb in rf.VARIANTS:
        args = (x, s if aff else None, t if aff else None, w, bias if hb else None, act)
        got = _run(engine, ops, B, act, aff, hb, p)
        want, bnd = rf.f64(*args), rf.bound(*args)
        _judge(got, want, bnd, f"rows_fc path {p} Cin {Cin} Nout {Nout} act {act} {name}")
        if act == 2:
            # the sigmoid in isolation: against float64 on the kernel's OWN fp32 pre-activation (act 0 differs in the last step only)
            v32 = _run(engine, ops, B, 0, aff, hb, p)
            sig = np.abs(got - 1.0 / (1.0 + np.exp(-v32))) / rf.sigmoid_bound(v32)
            print(f"    pre-activations in [{v32.min():.1f}, {v32.max():.1f}]; the sigmoid alone: worst err / ((|v| + 8) 2^-24) {float(sig.max()):.3g}")
            assert sig.max() <= 1, f"path {p} {name}: 1 / (1 + __expf(-v)) outside the figure of tests/sweeps_ref.py, worst err / bound {float(sig.max()):.3g}"


PROPERTY_CASES = [(3, 2944, 192), (2, 2432, 70), (1, 224, 200), (0, 1000, 33)]


@pytest.mark.parametrize("p,Cin,Nout", PROPERTY_CASES)
def test_reproducible_row_independent_and_nan_isolating(engine, p, Cin, Nout):
    B = 9 if p == 0 else 65
    rows = (0, 3, 4, 8) if p == 0 else (0, 1, 31, 32, 64)
    for act in (0, 2):
        x, s, t, w, bias = rf.real_operands(Cin, Nout, B, act, seed=1)
        ops = Operands(x, s, t, w, bias)
        for name, aff, hb in rf.VARIANTS:
            a = _run(engine, ops, B, act, aff, hb, p)
            assert np.isfinite(a).all()
            assert np.array_equal(a, _run(engine, ops, B, act, aff, hb, p)), f"path {p} {name}: two calls differ"
            for r in rows:                                             # _run asserts that the slice stays on the path (16-byte aligned rows)
                one = _run(engine, ops, 1, act, aff, hb, p, row0=r)
                assert np.array_equal(one[0], a[r]), f"path {p} {name} act {act}: row {r} alone differs from row {r} of the batch of {B}"
        r_nan = rows[-2]
        xn = x.copy()
        xn[r_nan, Cin // 3] = np.nan
        opn = Operands(xn, s, t, w, bias)
        for name, aff, hb in rf.VARIANTS:
            clean, dirty = _run(engine, ops, B, act, aff, hb, p), _run(engine, opn, B, act, aff, hb, p)
            assert np.isnan(dirty[r_nan]).all(), f"path {p} {name} act {act}: the NaN row must be NaN"
            keep = np.arange(B) != r_nan
            assert np.array_equal(clean[keep], dirty[keep]), f"path {p} {name} act {act}: a NaN in row {r_nan} changed another row"


def test_refusals_launch_nothing(engine):
    x, s, t, w, bias = rf.int_operands(128, 64, 4)
    ops = Operands(x, s, t, w, bias)
    buf = torch.full((4 + 3, 64), SENT, dtype=torch.float32, device="cuda")

    def call(x_ptr=ops.x.data_ptr(), s_=ops.s, t_=ops.t, w_ptr=ops.w.data_ptr(), out=buf, B=4, Cin=128, Nout=64, act=0):
        return _raw(engine, x_ptr, 128, s_, t_, w_ptr, ops.bias, out, B, Cin, Nout, act)

    for kw, msg in ((dict(x_ptr=None), "null argument"), (dict(w_ptr=None), "null argument"), (dict(B=0), "empty problem"), (dict(Cin=0), "empty problem"),
                    (dict(Nout=0), "empty problem"), (dict(act=3), "act=3"), (dict(act=-1), "act=-1"), (dict(t_=None), "go together"),
                    (dict(s_=None), "go together")):
        with pytest.raises(L.SdkError, match=msg):
            L.check(call(**kw), "sdk_rows_fc")
    torch.cuda.synchronize()
    assert (buf == SENT).all(), "a refused call wrote to the output"
    assert call() == 0                                                 # the same arguments, unmodified, are accepted
    torch.cuda.synchronize()
    assert np.array_equal(buf[:4].cpu().numpy().astype(np.float64), rf.exact(x, s, t, w, bias, 0).astype(np.float64)) and (buf[4:] == SENT).all()
