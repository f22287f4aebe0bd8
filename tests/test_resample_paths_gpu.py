"""sdk_resample_s16 (csrc/resample.hip) on each of its four instantiations resample_kernel<LDS_TAPS, LDS_WIN>, bit for bit.

Every case states the instantiation it runs and proves it with sdk_resample_plan, the function the launch is decided by.  Every output is
compared with the vectorised oracle (oracle/resample.py) and a sampled set - the first and last K outputs, those around the 2048-output
workgroup edges, 200 seeded ones - with the scalar Python-integer reference (tests/resample_ref.py).  Synthetic tap tables go straight to the
C ABI, with y inside a sentinel-filled buffer that must stay untouched on both sides; designed ones go through Engine.resample_s16.
tests/test_resample_ref_cpu.py shows on the reference alone that the fixtures used here saturate, tie and round as each test needs.
Nothing here has a tolerance."""
import numpy as np
import pytest
import torch

import resample_ref as rr
from conftest import sub
from oracle import resample as ors

pytestmark = pytest.mark.gpu

LIB = sub("_lib")
SENT = 0x5A5A                  # sentinel around y
GUARD = 64                     # sentinel elements on each side of y
ROWS = {c[0]: c for c in rr.CASES}


def tables(shape):
    """-> (taps int32 [L, K], rate or None) of a row of the case table; the row's plan value is asserted on the way."""
    (L, M, K), rate, lds_taps, lds_win = ROWS[shape]
    assert LIB.load_library().sdk_resample_plan(L, M, K) == (1 if lds_taps else 0) | (2 if lds_win else 0)
    if rate is None:
        return rr.synthetic_taps(L, M, K), None
    taps, Ld, Md, Kd = ors.design_taps(rate, 16000)
    assert (Ld, Md, Kd) == (L, M, K)
    return taps, rate


def dev(a):
    return a if isinstance(a, torch.Tensor) else torch.from_numpy(np.array(a)).cuda()      # a copy: designed tables are read-only


def abi(engine, x, taps, L, M, K) -> torch.Tensor:
    """x [n] or [n, C] and taps through the C ABI on the current stream; y sits between two sentinel stretches, which must come back whole."""
    xd, td = dev(x), dev(np.asarray(taps, dtype=np.int32))
    n_in, ch = xd.shape[0], (1 if xd.dim() == 1 else xd.shape[1])
    n_out = rr.out_len(n_in, L, M)
    buf = torch.full((GUARD + n_out + GUARD,), SENT, dtype=torch.int16, device="cuda")
    y = buf[GUARD:GUARD + n_out]
    LIB.check(engine.lib.sdk_resample_s16(engine.ctx, xd.data_ptr(), n_in, ch, td.data_ptr(), L, M, K, y.data_ptr(), n_out,
                                          torch.cuda.current_stream().cuda_stream), "sdk_resample_s16")
    torch.cuda.current_stream().synchronize()
    assert (buf[:GUARD] == SENT).all() and (buf[GUARD + n_out:] == SENT).all(), "wrote outside y"
    return y


def run(engine, shape, x, taps, rate) -> np.ndarray:
    L, M, K = shape
    y = abi(engine, x, taps, L, M, K) if rate is None else engine.resample_s16(dev(x), rate, 16000)
    torch.cuda.synchronize()
    assert y.dtype == torch.int16 and y.shape == (rr.out_len(len(x), L, M),)
    return y.cpu().numpy()


def compare(got, x, taps, L, M, every=False):
    want = ors.resample_s16(x, taps, L, M)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{bad.size} of {len(want)} outputs differ from the oracle, first at {bad[:5].tolist()}: got {got[bad[:5]].tolist()}, want {want[bad[:5]].tolist()}"
    idx = list(range(len(got))) if every else rr.sample_indices(len(got), taps.shape[1])
    ref = rr.resample_at(x, taps, L, M, idx)
    assert got[idx].tolist() == ref, [(n, int(got[n]), r) for n, r in zip(idx, ref) if got[n] != r][:5]


@pytest.mark.parametrize("kind", ["edges", "short"])
@pytest.mark.parametrize("shape", [c[0] for c in rr.CASES], ids=rr.case_id)
def test_lengths(engine, shape, kind):
    """`edges`: mono input whose output ends one before, at and one past a workgroup edge, and one past the second (n_out 1, 2047, 2048, 2049,
    4097; on the interpolating row 4100, 3, 4 the reachable lengths 1367, 2734, 4100).  `short`: 3-channel input of 1, 2, K/2 - 1, K/2, K
    and K + 1 frames, the windows that hang over both ends of the signal at once."""
    L, M, K = shape
    taps, rate = tables(shape)
    edges, short = rr.lengths(L, M, K)
    for n_in in (edges if kind == "edges" else short):
        x = rr.noise(n_in, 0 if kind == "edges" else 3, [L, M, K, n_in])
        compare(run(engine, shape, x, taps, rate), x, taps, L, M)


@pytest.mark.parametrize("shape", rr.SATURATION, ids=rr.case_id)
def test_forced_saturation(engine, shape):
    """Under every target output the input is +-32767 sign(h): the accumulator is the largest its phase can reach, alternately positive and
    negative, and the reference clamps it on both sides (test_resample_ref_cpu.py asserts that it does)."""
    L, M, K = shape
    taps, rate = tables(shape)
    x, targets = rr.saturation_input(taps, L, M)
    got = run(engine, shape, x, taps, rate)
    raw = rr.resample_raw_at(x, taps, L, M, targets)
    hi = [n for n, v in zip(targets, raw) if v > 32767]
    lo = [n for n, v in zip(targets, raw) if v < -32768]
    assert len(hi) >= 4 and len(lo) >= 4
    assert (got[hi] == 32767).all() and (got[lo] == -32768).all(), (got[hi].tolist(), got[lo].tolist())
    assert got[targets].tolist() == rr.resample_at(x, taps, L, M, targets)
    compare(got, x, taps, L, M)


@pytest.mark.parametrize("shape,name", [((1, 1, 2), "half"), ((1, 1, 2), "neg_half"), ((1, 1, 2), "sum"), ((1, 17, 2), "half")],
                         ids=["lds_half", "lds_neg_half", "lds_sum", "global_half"])
def test_all_s16_values_through_the_rounding(engine, shape, name):
    """Taps 2^29 and -2^29 put every odd sample exactly half way, on both signs: round half up.  Taps (2^30, 2^30) add neighbours: both
    clamps and the values next to them.  With M = 17 the window is read from global memory; the values tiled 17 times put each under tap 0."""
    L, M, K = shape
    tables(shape)
    taps = np.array(rr.ROUNDING_TABLES[name], dtype=np.int32)
    x = rr.all_s16_values()
    if M == 17:
        x = np.tile(x, 17)
    got = abi(engine, x, taps, L, M, K).cpu().numpy()
    compare(got, x, taps, L, M, every=True)
    if name == "half":                                               # (v + 1) >> 1 for every s16 value v, in closed form as well
        v = x[::M][:len(got)].astype(np.int64)
        assert np.array_equal(got, (v + 1) >> 1)
        assert sorted(set(v.tolist())) == list(range(-32768, 32768))


@pytest.mark.parametrize("path", ["lds_window", "global_window"])
@pytest.mark.parametrize("ch", rr.CHANNELS)
def test_downmix(engine, ch, path):
    """floor((sum + C // 2) / C) on rows that tell floor from truncation and need the rounding term, up to the 64 channels the ABI admits.
    `lds_window`: through the window fill (identity table: y is the down-mix itself) and a designed filter at 250 kHz.  `global_window`:
    through the per-tap read (M = 17 with the identity table: every 17th down-mixed sample) and a designed filter at 264.6 kHz, where the
    taps are global as well."""
    x = rr.downmix_input(ch)
    mono = np.array(rr.downmix(x), dtype=np.int16)
    ident = np.array([[1 << 30, 0]], dtype=np.int32)
    L, M, K = (1, 1, 2) if path == "lds_window" else (1, 17, 2)
    designed = (8, 125, 500) if path == "lds_window" else (80, 1323, 530)
    tables((L, M, K))
    got = abi(engine, x, ident, L, M, K).cpu().numpy()
    assert np.array_equal(got, mono[::M])
    compare(got, x, ident, L, M, every=True)
    taps, rate = tables(designed)
    got = engine.resample_s16(dev(x), rate, 16000).cpu().numpy()
    compare(got, x, taps, designed[0], designed[1], every=True)
    if ch == 1:                                                      # [n] and [n, 1] are the same input
        for r in (16000, rate):
            assert torch.equal(engine.resample_s16(dev(x), r, 16000), engine.resample_s16(dev(x[:, 0].copy()), r, 16000))


@pytest.mark.parametrize("path", ["lds_window", "global_window"])
def test_element_index_past_2_31(engine, path):
    """x [2^25 + 2049, 64]: the interleaved index of the last frames exceeds 2^31 (4.0 GiB of int16).  Zeros, then 4096 frames of noise:
    the tail must equal the reference run on the tail alone, and the zero stretch must come out as zeros.  `lds_window`: the identity
    table, y is the down-mix.  `global_window`: M = 17, output n reads the frames 17 n and 17 n + 1 tap by tap."""
    free, _ = torch.cuda.mem_get_info()
    if free < 6 << 30:
        pytest.skip(f"needs 6 GiB of free device memory for a 4 GiB input, {free / 2 ** 30:.1f} GiB free")
    N, ch, T = (1 << 25) + 2049, 64, 4096
    assert N * ch > 1 << 31 > (N - T) * ch                           # the noise straddles element 2^31
    tail = rr.noise(T, ch, 2031)
    rng = np.random.default_rng(2032)
    x = torch.zeros((N, ch), dtype=torch.int16, device="cuda")
    x[N - T:] = torch.from_numpy(tail).cuda()
    try:
        if path == "lds_window":
            ident = np.array([[1 << 30, 0]], dtype=np.int32)
            tables((1, 1, 2))
            y = abi(engine, x, ident, 1, 1, 2)
            assert y.shape == (N,)
            got = y[N - T:].cpu().numpy()
            assert np.array_equal(got, ors.resample_s16(tail, ident, 1, 1)) and got.tolist() == rr.downmix(tail) and np.abs(got).max() > 1000
            nz = N - T                                               # outputs below this read zeros only (tap 1 is zero)
        else:
            taps, _ = tables((1, 17, 2))
            y = abi(engine, x, taps, 1, 17, 2)
            a = -(-(N - T) // 17) * 17                               # first frame of the tail that starts an output
            seg = tail[a - (N - T):]
            want = ors.resample_s16(seg, taps, 1, 17)
            assert y.shape == (rr.out_len(N, 1, 17),) and len(want) == len(y) - a // 17
            got = y[a // 17:].cpu().numpy()
            assert np.array_equal(got, want) and got.tolist() == rr.resample_at(seg, taps, 1, 17, range(len(want))) and np.abs(got).max() > 1000
            nz = (N - T) // 17 - 1                                   # outputs below this read zeros only
        zi = torch.from_numpy(np.concatenate([rng.integers(0, nz, 996), [0, 2047, 2048, nz - 1]])).cuda()
        assert not y[zi].any() and not y[:nz].any()
    finally:
        del x
        torch.cuda.empty_cache()


@pytest.mark.parametrize("shape,rate", rr.DESIGNED, ids=[rr.case_id(s) for s, _ in rr.DESIGNED])
def test_noise_at_designed_rates(engine, shape, rate):
    """2400 stereo frames of full-scale noise at each designed rate: twice on the default stream, once on another, once through the C ABI with
    the host's own table inside sentinels - the same bits each time, those of the reference."""
    L, M, K = shape
    taps, _ = tables(shape)
    x = rr.noise(2400, 2, [rate, 2400])
    xd = dev(x)
    first = engine.resample_s16(xd, rate, 16000)
    second = engine.resample_s16(xd, rate, 16000)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        third = engine.resample_s16(xd, rate, 16000)
        fourth = abi(engine, xd, sub("resample").design_taps(rate, 16000)[0], L, M, K)
    side.synchronize()
    assert torch.equal(first, second) and torch.equal(first, third) and torch.equal(first, fourth)
    compare(first.cpu().numpy(), x, taps, L, M)


def _valid_call_equals_reference(engine):
    x = rr.noise(40, 2, 404)
    taps = rr.synthetic_taps(1, 1, 2)
    compare(abi(engine, x, taps, 1, 1, 2).cpu().numpy(), x, taps, 1, 1, every=True)


REFUSALS = {           # name -> (overrides of the valid call, what the message must name)
    "null_ctx": ({"ctx": None}, "null"), "null_x": ({"x": None}, "null"), "null_taps": ({"taps": None}, "null"), "null_y": ({"y": None}, "null"),
    "n_in_0": ({"n_in": 0, "n_out": 0}, "n_in=0"), "channels_0": ({"ch": 0}, "channels=0"), "channels_65": ({"ch": 65}, "channels=65"),
    "L_0": ({"L": 0}, "L=0"), "M_0": ({"M": 0}, "M=0"), "K_0": ({"K": 0}, "K=0"), "K_1": ({"K": 1}, "K=1"), "K_3": ({"K": 3}, "K=3"),
    "LK_over": ({"L": (1 << 21) + 1, "n_out": 16 * ((1 << 21) + 1)}, "L=2097153"),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refusals(engine, name):
    """Each refused call returns nonzero with a message that names the offending value, launches nothing (a sentinel-filled y stays whole)
    and leaves the context usable.  Every buffer is as large as the refused arguments describe, so the call stays in bounds whatever it does.
    (n_in >= 2^40 is left to reading: a test of it would hand the kernel a length its buffer does not have.)"""
    over, token = REFUSALS[name]
    a = {"ctx": engine.ctx, "n_in": 16, "ch": 1, "L": 1, "M": 1, "K": 2, "n_out": 16}
    a.update({k: v for k, v in over.items() if k not in ("x", "taps", "y")})
    x = torch.zeros((16 * max(a["ch"], 1),), dtype=torch.int16, device="cuda")
    taps = torch.zeros((max(a["L"], 1) * max(a["K"], 2),), dtype=torch.int32, device="cuda")
    y = torch.full((max(a["n_out"], 16) + GUARD,), SENT, dtype=torch.int16, device="cuda")
    ptr = {k: (None if k in over else t.data_ptr()) for k, t in (("x", x), ("taps", taps), ("y", y))}
    lib = engine.lib
    rc = lib.sdk_resample_s16(a["ctx"], ptr["x"], a["n_in"], a["ch"], ptr["taps"], a["L"], a["M"], a["K"], ptr["y"], a["n_out"], 0)
    msg = lib.sdk_last_error().decode()
    torch.cuda.synchronize()
    assert rc != 0 and msg.startswith("sdk_resample_s16") and token in msg, (rc, msg)
    assert (y == SENT).all()
    with pytest.raises(LIB.SdkError, match=token):
        LIB.check(rc, "sdk_resample_s16")
    _valid_call_equals_reference(engine)


def test_wrapper_refuses_what_it_cannot_read(engine):
    """Engine.resample_s16 names its argument: an empty input, a 3-D tensor (once read as [n, C] with the third extent ignored) and a tensor
    that is not int16.  A valid call right after is served."""
    with pytest.raises(ValueError, match=r"resample_s16: x must be int16 \[n\] or \[n, C\] with n >= 1, got \[0\]"):
        engine.resample_s16(torch.zeros((0,), dtype=torch.int16, device="cuda"), 48000)
    with pytest.raises(ValueError, match=r"resample_s16: x must be .* got \[0, 2\]"):
        engine.resample_s16(torch.zeros((0, 2), dtype=torch.int16, device="cuda"), 48000)
    with pytest.raises(ValueError, match=r"resample_s16: x must be .* got \[10, 2, 3\]"):
        engine.resample_s16(torch.zeros((10, 2, 3), dtype=torch.int16, device="cuda"), 48000)
    with pytest.raises(LIB.SdkError, match=r"x must be torch.int16, got torch.float32"):
        engine.resample_s16(torch.zeros((10,), dtype=torch.float32, device="cuda"), 48000)
    with pytest.raises(LIB.SdkError, match=r"x must live in device memory"):
        engine.resample_s16(torch.zeros((10,), dtype=torch.int16), 48000)
    x = rr.noise(100, 2, 9)
    taps, L, M, K = ors.design_taps(48000, 16000)
    compare(engine.resample_s16(dev(x), 48000).cpu().numpy(), x, taps, L, M, every=True)
