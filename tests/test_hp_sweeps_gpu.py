"""The precise mode's four sweeps (csrc/hp.hip: sdk_seg_mean_hp, sdk_se_apply_hp, sdk_asp_stats_hp, sdk_asp_pool_hp), each kernel on
its own against the float64 restatements of tests/hp_ref.py on the values the planes hold.  Shapes sit on the kernels' channel
blocks (512 / 1024 / 256 wide, one 8-channel chunk either side), on the frame groups (T < 4, T % 8) and on more than one block; the
data include magnitudes the lo plane carries alone, saturation, a transient frame 0, constant columns and logits that rescale the
online softmax on every frame or never.  Inputs are views into wider sentinel-filled buffers, outputs sit inside sentinel-filled
buffers that must come back untouched.  Every comparison is element-wise over every element, |got - want| <= bound with
bound = n 2^-24 sum|terms| (hp_ref); each case prints its worst error / bound."""
import pytest
import torch

import hp_ref as H
from conftest import sub

pytestmark = pytest.mark.gpu

L = sub("_lib")
SdkError = L.SdkError
B = 3
PAD = 32                # fp32 sentinel elements either side of an fp32 output


def judge(got, want, bound, what):
    """|got - want| <= bound element-wise, every element (a NaN anywhere fails); prints and returns the worst error / bound"""
    got = got.double().cpu()
    assert got.shape == want.shape == bound.shape, (got.shape, want.shape, bound.shape)
    err = (got - want).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    bad = ~(err <= bound)
    print(f"{what}: worst err / bound {ratio:.3f}")
    assert not bad.any(), f"{what}: {int(bad.sum())} / {bad.numel()} outside the bound, worst err / bound {ratio:.3g}"
    return ratio


def _operand(v, pad_lo, pad_ld):
    """fp32 [rows, C] -> (device view of the planes, lo offset): lo = C + pad_lo > C, ld = lo + C + pad_ld > lo + C, two spare rows"""
    rows, C = v.shape
    lo = C + pad_lo
    return H.planes(v, lo + C + pad_ld, lo, rows_extra=2).cuda()[:rows], lo


def _f32_out(n):
    """a contiguous fp32 output of n elements inside a sentinel-filled buffer"""
    flat = torch.full((n + 2 * PAD,), H.SENT, dtype=torch.float32, device="cuda")
    return flat, flat[PAD:PAD + n]


def _f32_untouched(flat, what):
    f = flat.cpu()
    assert (f[:PAD] == H.SENT).all() and (f[-PAD:] == H.SENT).all(), f"{what}: store outside the output"


# ---------------------------------------------------------------------------------------------------- seg_mean_hp
@pytest.mark.parametrize("C", [8, 504, 512, 520, 1024, 1536])
def test_seg_mean_hp(engine, C):
    """the 512-channel blocks and their guard; T below, at and past the four frame groups; |z| ~ 1e-5 (hi is subnormal: the lo plane
    carries the value) and constant columns"""
    for T in (1, 2, 3, 4, 5, 201):
        for kind in ("random", "small", "constant"):
            g = torch.Generator().manual_seed(C * 7 + T)
            z = torch.randn(B * T, C, generator=g) * (1e-5 if kind == "small" else 2.0) + (0.0 if kind == "small" else 0.5)
            if kind == "constant":
                z[:, ::3] = torch.randn(C, generator=g)[::3] * 4
            zp, lo = _operand(z, 8, 16)
            flat, out = _f32_out(B * C)
            engine.seg_mean_hp(zp, lo, B, T, C, out=out.view(B, C))
            torch.cuda.synchronize()
            want, bound = H.seg_mean_ref(H.decode(z), B, T)
            judge(out.view(B, C), want, bound, f"seg_mean_hp C {C} T {T} {kind}")
            _f32_untouched(flat, f"seg_mean_hp C {C} T {T}")


# ---------------------------------------------------------------------------------------------------- se_apply_hp
def _slab(rows, C):
    """the output as a column slab in the middle of a wider two-plane buffer, as in the forward's concatenation buffer: plane width
    Cw = 16 + C + 24, hi slab at columns [16, 16 + C), lo slab Cw further right; sentinels everywhere else, three spare rows"""
    off, Cw = 16, 16 + C + 24
    buf = torch.full((rows + 3, 2 * Cw), H.SENT, dtype=torch.float16, device="cuda")
    return buf, buf[:rows, off:], Cw, off


def _slab_check(buf, rows, C, Cw, off, what):
    b = buf.cpu()
    hi, lo = b[:rows, off:off + C].clone(), b[:rows, Cw + off:Cw + off + C].clone()
    b[:rows, off:off + C] = H.SENT
    b[:rows, Cw + off:Cw + off + C] = H.SENT
    assert (b == H.SENT).all(), f"{what}: store outside the output slab"
    return hi, lo


@pytest.mark.parametrize("C", [8, 24, 256, 1024, 1032])
def test_se_apply_hp(engine, C):
    """nch8 = 1 (a frame row far narrower than the workgroup), 3 (no power of two), 32, 128 and 129; T around the 8-frame block; z, x
    and out with a different ld / lo each; saturation at T = 9 and 201 (g z + x past +-65504 in a few elements: +-65504 exactly,
    lo = 0, no NaN); magnitude 1e-5 at T = 7"""
    for T in (1, 7, 8, 9, 201):
        g = torch.Generator().manual_seed(C * 11 + T)
        mag = 1e-5 if T == 7 else 1.0
        z = torch.randn(B * T, C, generator=g) * 2 * mag
        x = torch.randn(B * T, C, generator=g) * mag
        gate = torch.rand(B, C, generator=g)
        sat = T in (9, 201)
        if sat:
            rows = torch.tensor([T // 2, T + 1, B * T - 1])
            z[rows, :4] = 60000.0
            x[rows, :4] = 60000.0
            z[rows, 4:8] = -60000.0
            x[rows, 4:8] = -60000.0
            gate[:, :8] = 0.9
        zp, zlo = _operand(z, 8, 16)
        xp, xlo = _operand(x, 16, 8)
        buf, out, Cw, off = _slab(B * T, C)
        engine.se_apply_hp(zp, zlo, xp, xlo, gate.cuda(), out, Cw, B, T, C)
        torch.cuda.synchronize()
        what = f"se_apply_hp C {C} T {T}" + (" saturating" if sat else "") + (" small" if T == 7 else "")
        hi, lo = _slab_check(buf, B * T, C, Cw, off, what)
        tgt, bound, pre, acc = H.se_apply_ref(H.decode(z), H.decode(x), gate, B, T)
        judge(H.join(hi, lo), tgt, bound, what)
        over = pre.abs() - acc > H.HP_MAX
        assert int(over.sum()) == (3 * 8 if sat else 0)
        assert (hi[over].double() == torch.sign(pre[over]) * H.HP_MAX).all() and (lo[over] == 0).all(), f"{what}: saturated pairs"


# ---------------------------------------------------------------------------------------------------- asp_stats_hp
@pytest.mark.parametrize("C", [8, 1016, 1024, 1032, 1536, 3072])
def test_asp_stats_hp(engine, C):
    """the 1024-channel blocks and their guard, the two frame groups (T = 1, 2, 3); random data with constant columns (the variance
    floor); a transient frame 0 (frame 0 ~ 100, the rest ~ 0.01: the kernel shifts by frame 0)"""
    for T in (1, 2, 3, 201, 501):
        for kind in ("random", "transient"):
            g = torch.Generator().manual_seed(C * 13 + T)
            if kind == "random":
                h = torch.randn(B * T, C, generator=g) * 3 + 1
                h[:, ::5] = torch.randn(C, generator=g)[::5] * 4
            else:
                h = torch.randn(B * T, C, generator=g) * 0.01
                h.view(B, T, C)[:, 0] = 100 + torch.randn(B, C, generator=g)
            hp, lo = _operand(h, 8, 16)
            flat, out = _f32_out(B * 2 * C)
            engine.asp_stats_hp(hp, lo, B, T, C, out=out.view(B, 2 * C))
            torch.cuda.synchronize()
            want, bound = H.asp_stats_ref(H.decode(h), B, T)
            judge(out.view(B, 2 * C), want, bound, f"asp_stats_hp C {C} T {T} {kind}")
            _f32_untouched(flat, f"asp_stats_hp C {C} T {T}")


# ---------------------------------------------------------------------------------------------------- asp_pool_hp
LOGIT_KINDS = ["normal", "ascending", "descending", "peak", "equal", "offset", "tail"]


def _logits(kind, T, C, g):
    t = torch.arange(T, dtype=torch.float32)[None, :, None]
    lg = torch.randn(B, T, C, generator=g) * 3
    if kind == "ascending":                      # a rescale on every frame
        lg = t * 0.05 + torch.rand(B, 1, C, generator=g)
    elif kind == "descending":                   # never a rescale after the first frame
        lg = -t * 0.05 + torch.rand(B, 1, C, generator=g)
    elif kind == "peak":                         # one frame 80 above the rest
        lg = torch.randn(B, T, C, generator=g)
        lg[:, T // 3] += 80
    elif kind == "equal":
        lg = torch.full((B, T, C), 1.5)
    elif kind == "offset":                       # the max-subtraction
        lg = lg + 1e4
    elif kind == "tail" and T > 1:               # the last frames at -1e4
        lg[:, T - max(1, T // 4):] = -1e4
    return lg.reshape(B * T, C).contiguous()


@pytest.mark.parametrize("kind", LOGIT_KINDS)
@pytest.mark.parametrize("C", [8, 248, 256, 264, 1536, 3072])
def test_asp_pool_hp(engine, C, kind):
    """the 256-channel blocks and their guard; logits with ldl > C; the online softmax with a rescale on every frame, on none, across
    an 80-wide gap, at a common offset of 1e4 and with frames whose weight is exactly zero"""
    for T in (1, 2, 201, 501):
        g = torch.Generator().manual_seed(C * 17 + T)
        lg = _logits(kind, T, C, g)
        if kind == "ascending":
            assert (lg.view(B, T, C)[:, 1:] > lg.view(B, T, C)[:, :-1]).all()
        if kind == "descending":
            assert (lg.view(B, T, C)[:, 1:] < lg.view(B, T, C)[:, :-1]).all()
        h = torch.randn(B * T, C, generator=g) * 2 + 3
        hp, lo = _operand(h, 8, 16)
        lw = torch.full((B * T + 1, C + 8), H.SENT, dtype=torch.float32)
        lw[:B * T, :C] = lg
        flat, out = _f32_out(B * 2 * C)
        engine.asp_pool_hp(lw.cuda()[:B * T, :C], hp, lo, B, T, C, out=out.view(B, 2 * C))
        torch.cuda.synchronize()
        want, bound = H.asp_pool_ref(lg, H.decode(h), B, T)
        judge(out.view(B, 2 * C), want, bound, f"asp_pool_hp C {C} T {T} {kind}")
        _f32_untouched(flat, f"asp_pool_hp C {C} T {T} {kind}")


# ---------------------------------------------------------------------------------------------------- refusals
def test_sweep_entry_points_refuse_malformed_arguments(engine):
    """C = 12, a lo offset of 4, ld < lo + C, a pointer off the 16-byte grid, B = 0: each refused by name with nothing launched (every
    operand below would stay inside its buffer even so), and a valid call afterwards still gives the right answer"""
    T, C = 5, 16
    g = torch.Generator().manual_seed(1)
    z, x = torch.randn(B * T, C, generator=g), torch.randn(B * T, C, generator=g)
    gate = torch.rand(B, C, generator=g)
    lg = torch.randn(B * T, C, generator=g)
    zp, lo = _operand(z, 8, 16)
    xp, xlo = _operand(x, 16, 8)
    narrow = torch.zeros(B * T + 4, 24, dtype=torch.float16, device="cuda")[:B * T]            # ld = 24 < lo + C = 32
    odd = torch.zeros(B * T + 4, 64, dtype=torch.float16, device="cuda")[:B * T, 1:]            # two bytes off the grid
    dg, dl = gate.cuda(), lg.cuda()
    buf, out, Cw, off = _slab(B * T, C)
    flat, o32 = _f32_out(B * 2 * C)                  # (an output the method would size by B = 0 has no address: given here instead)
    calls = {
        "sdk_seg_mean_hp": lambda p, l, b, c: engine.seg_mean_hp(p, l, b, T, c, out=o32),
        "sdk_se_apply_hp": lambda p, l, b, c: engine.se_apply_hp(p, l, xp, xlo, dg, out, Cw, b, T, c),
        "sdk_asp_stats_hp": lambda p, l, b, c: engine.asp_stats_hp(p, l, b, T, c, out=o32),
        "sdk_asp_pool_hp": lambda p, l, b, c: engine.asp_pool_hp(dl, p, l, b, T, c, out=o32),
    }
    for name, call in calls.items():
        for args, msg in (((zp, lo, B, 12), "C=12"), ((zp, 4, B, C), "lo=4"), ((narrow, 16, B, C), "ld=24"), ((odd, lo, B, C), "16-byte aligned"),
                          ((zp, lo, 0, C), "B=0")):
            with pytest.raises(SdkError, match=f"{name}: .*{msg}"):
                call(*args)
    # se_apply's other operands and the logits' row length
    with pytest.raises(SdkError, match="sdk_se_apply_hp: bad x planes: .*lo=4"):
        engine.se_apply_hp(zp, lo, xp, 4, dg, out, Cw, B, T, C)
    with pytest.raises(SdkError, match="sdk_se_apply_hp: bad out planes: .*lo=8"):
        engine.se_apply_hp(zp, lo, xp, xlo, dg, out, 8, B, T, C)
    with pytest.raises(SdkError, match="sdk_asp_pool_hp: ldl=8"):
        engine.asp_pool_hp(torch.zeros(B * T + 4, 8, device="cuda")[:B * T], zp, lo, B, T, C)
    with pytest.raises(SdkError, match="sdk_seg_mean_hp: null argument"):
        L.check(engine.lib.sdk_seg_mean_hp(engine.ctx, None, 64, 24, B, T, C, dg.data_ptr(), None), "sdk_seg_mean_hp")
    torch.cuda.synchronize()
    assert (buf.cpu() == H.SENT).all() and (flat.cpu() == H.SENT).all(), "a refused call stored"
    # ... and valid calls still work
    zd, xd = H.decode(z), H.decode(x)
    want, bound = H.seg_mean_ref(zd, B, T)
    judge(engine.seg_mean_hp(zp, lo, B, T, C), want, bound, "seg_mean_hp after the refusals")
    engine.se_apply_hp(zp, lo, xp, xlo, dg, out, Cw, B, T, C)
    torch.cuda.synchronize()
    hi, l = _slab_check(buf, B * T, C, Cw, off, "se_apply_hp after the refusals")
    tgt, bound, _, _ = H.se_apply_ref(zd, xd, gate, B, T)
    judge(H.join(hi, l), tgt, bound, "se_apply_hp after the refusals")
    want, bound = H.asp_stats_ref(zd, B, T)
    judge(engine.asp_stats_hp(zp, lo, B, T, C), want, bound, "asp_stats_hp after the refusals")
    want, bound = H.asp_pool_ref(lg, zd, B, T)
    judge(engine.asp_pool_hp(dl, zp, lo, B, T, C), want, bound, "asp_pool_hp after the refusals")
