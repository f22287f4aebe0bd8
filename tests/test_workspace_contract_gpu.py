"""The C ABI's promise about scratch memory, entry point by entry point (tests/ws_contract.py holds the harness and the table): a workspace of
exactly sdk_*_workspace_bytes bytes, whatever it holds, gives the same bytes; stale state of a larger shape in the same buffer changes
nothing; the public wrapper (cached, oversized scratch) returns the same bytes; one byte short is refused before any launch.  The wrappers
are pinned to float64 or exact references by the other GPU tests, so equality with them ties the exact-size path to those references.
The stream state block of sdk_stream_* gets the same treatment below."""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ws_contract as WC  # noqa: E402

pytestmark = pytest.mark.gpu
NAMES = sorted(WC.CASES)


def _err(engine) -> str:
    return (engine.lib.sdk_last_error() or b"").decode()


@pytest.mark.parametrize("name", NAMES)
def test_contents_do_not_matter(engine, name):
    """(a) 0xFF, 0x00 and random bytes in an exact-size workspace: rc 0, the same output bytes, every element the header documents as written
    is written, both guards and every output tail intact."""
    c = WC.case(engine, name)
    need = c.need(engine)
    ref = None
    for fill in WC.FILLS:
        g = WC.guarded(need, fill)
        rc, bufs = c.run(engine, g.ptr, g.need)
        assert rc == 0, (c.name, fill, rc, _err(engine))
        assert g.intact(), f"{c.name} [{fill}]: a guard around the {need}-byte workspace was written"
        masks = c.masks(bufs)
        for out, b in bufs.items():
            assert b.tail_intact(), f"{c.name} [{fill}]: {out} was written past its documented size"
            if out not in c.pre:
                stale = (b.host()[masks[out]] == WC.SENTINEL_BYTE).all(axis=1)
                assert not stale.any(), f"{c.name} [{fill}]: {int(stale.sum())} documented elements of {out} were not written, first {np.flatnonzero(stale)[:4].tolist()}"
        got = WC.written_bytes(c, bufs)
        ref = got if ref is None else ref
        for out in got:
            assert got[out] == ref[out], f"{c.name}: {out} differs between the {WC.FILLS[0]} fill and the {fill} fill"
        if c.check is not None:
            assert c.check(c.typed(bufs)), f"{c.name}: the shape does not reach the path it stands for: {({k: v.reshape(-1)[:4].tolist() for k, v in c.typed(bufs).items()})}"


@pytest.mark.parametrize("name", NAMES)
def test_stale_state_of_a_larger_shape_does_not_matter(engine, name):
    """(b) what the cached scratch does in production: the larger sibling runs in a buffer, then the case in the same buffer, not refilled,
    with ws_bytes the smaller need."""
    c = WC.case(engine, name)
    big = c.big()
    need, need_big = c.need(engine), big.need(engine)
    assert need_big > need, (c.name, need, big.name, need_big)
    g = WC.guarded(need_big, "ff")
    rc, _ = big.run(engine, g.ptr, g.need)
    assert rc == 0 and g.intact(), (big.name, rc, _err(engine))
    rc, bufs = c.run(engine, g.ptr, need)
    assert rc == 0 and g.intact(), (c.name, rc, _err(engine))
    got, ref = WC.written_bytes(c, bufs), WC.reference_bytes(engine, name)
    for out in got:
        assert got[out] == ref[out], f"{c.name}: {out} differs after {big.name} ran in the same workspace"
        assert bufs[out].tail_intact()


@pytest.mark.parametrize("name", NAMES)
def test_the_wrapper_returns_the_same_bytes(engine, name):
    """(c) the public wrapper on the same inputs."""
    c = WC.case(engine, name)
    g = WC.guarded(c.need(engine), "random", seed=1)
    rc, bufs = c.run(engine, g.ptr, g.need)
    assert rc == 0 and g.intact(), (c.name, rc, _err(engine))
    got, want = WC.wrapper_bytes(c, bufs)
    assert got, c.name
    for out in got:
        assert got[out] == want[out], f"{c.name}: the wrapper's {out} differs from the exact-size call's"


@pytest.mark.parametrize("name", NAMES)
def test_one_byte_short_is_refused(engine, name):
    """(d) ws_bytes = need - 1: non-zero, sdk_last_error names both sizes, and nothing was launched."""
    c = WC.case(engine, name)
    need = c.need(engine)
    g = WC.guarded(need, "ff")
    rc, bufs = c.run(engine, g.ptr, need - 1)
    msg = _err(engine)
    assert rc != 0, f"{c.name}: a workspace of {need - 1} bytes was accepted ({need} needed)"
    assert str(need - 1) in msg and str(need) in msg and "sdk_" in msg, (c.name, msg)
    assert c.untouched(bufs) and g.intact(), f"{c.name}: an output or the workspace was written by a refused call"


# ------------------------------------------------------------------------------------------------ the stream state block
D, CAPACITY, HOP, LATENCY, R = 64, 4, 8000, 8000, 3


def _stream_state(engine, fill):
    """A StreamState of R streams whose block is an exact-size guarded buffer holding `fill`, NOT reset.  This depends on two things of
    ops_cluster.StreamState: its constructor (engine, R, capacity, d, nbytes) makes the output rows, and the wrappers read the block's address
    and size from its .buf and .nbytes alone - so replacing .buf with a slice of the same size puts the guarded block under every call."""
    oc = WC._sub("ops_cluster")
    nbytes = int(engine.lib.sdk_stream_state_bytes(R, CAPACITY, D))
    assert nbytes > 0
    g = WC.guarded(nbytes, fill)
    off = g.ptr - g.buf.data_ptr()
    st = oc.StreamState(engine, R, CAPACITY, D, nbytes)
    st.buf = g.buf[off:off + nbytes]
    return st, g


def _run_streams(engine, st, active=(1, 1, 1)):
    """The step sequence of test_stream_gpu.test_step_kernel_equals_the_reference on `st` -> the bytes of every output of every step, of the
    flush and of sdk_stream_centroids."""
    import test_stream_gpu as TS
    streams = [TS.stream_of(D, HOP, r % TS.N_DISTINCT) for r in range(R)]
    Cn = len(streams[0][0]["starts"])
    E_d = torch.from_numpy(np.stack([s["E"] for s, _ in streams], 1).copy()).cuda()
    info_d = torch.from_numpy(np.stack([s["info"] for s, _ in streams], 1)).cuda()
    cls_d = torch.from_numpy(np.stack([s["cls"] for s, _ in streams], 1)).cuda()
    starts_d = torch.from_numpy(np.stack([s["starts"] for s, _ in streams], 1)).cuda()
    on = torch.tensor(list(active), dtype=torch.uint8, device="cuda")
    ends = [n if (n < TS.CHUNK or (n - TS.CHUNK) % HOP) else 0 for _, n in streams]
    end_d = torch.tensor(ends, dtype=torch.int64, device="cuda")
    out = []
    for c in range(Cn):
        engine.stream_step(st, E_d[c].reshape(3 * R, D), info_d[c], cls_d[c], starts_d[c], on, HOP, LATENCY, TS.DELTA, None, end_d if c == Cn - 1 and any(ends) else None)
        out.append([t.cpu().numpy().copy() for t in (st.labels, st.score, st.K, st.emit_lo, st.emit_n, st.count, st.speakers)])
    engine.stream_flush(st, torch.tensor([n for _, n in streams], dtype=torch.int64, device="cuda"), on)
    out.append([t.cpu().numpy().copy() for t in (st.emit_lo, st.emit_n, st.count, st.speakers)])
    out.append([t.cpu().numpy().copy() for t in engine.stream_centroids(st, sums=True)])
    return out


def _same(a, b, rows=None):
    for sa, sb in zip(a, b):
        for x, y in zip(sa, sb):
            if (x.tobytes() if rows is None else x[rows].tobytes()) != (y.tobytes() if rows is None else y[rows].tobytes()):
                return False
    return len(a) == len(b)


def test_stream_reset_of_a_poisoned_block_equals_a_zeroed_one(engine):
    """sdk_stream_reset clears the header alone: after it a block of 0xFF must behave as a block of zeros, step by step, through the flush
    and in sdk_stream_centroids."""
    runs = []
    for fill in ("00", "ff"):
        st, g = _stream_state(engine, fill)
        engine.stream_reset(st)
        runs.append(_run_streams(engine, st))
        assert g.intact(), f"a guard around the state block was written ({fill})"
    assert _same(runs[0], runs[1]), "a reset block of 0xFF and a reset block of zeros give different bytes"
    assert int(runs[0][-1][2].min()) >= 1                                            # every stream founded a speaker: the run did something


def test_stream_reset_of_one_stream_leaves_the_others(engine):
    st, g = _stream_state(engine, "ff")
    per = st.nbytes // R
    which = torch.tensor([0, 1, 0], dtype=torch.uint8, device="cuda")
    engine.stream_reset(st, which)
    torch.cuda.synchronize()
    assert bool((st.buf[:per] == 0xFF).all()) and bool((st.buf[2 * per:] == 0xFF).all()), "the reset of stream 1 wrote stream 0 or 2"
    got = _run_streams(engine, st, active=(0, 1, 0))
    torch.cuda.synchronize()
    assert bool((st.buf[:per] == 0xFF).all()) and bool((st.buf[2 * per:] == 0xFF).all()) and g.intact()
    full, g2 = _stream_state(engine, "00")
    engine.stream_reset(full)
    want = _run_streams(engine, full)
    # stream 1's rows of every step and of the flush; centroids of stream 1 alone
    assert _same(got[:-1], want[:-1], rows=1) and g2.intact()
    for x, y in zip(engine.stream_centroids(st, first=1, count=1, sums=True), engine.stream_centroids(full, first=1, count=1, sums=True)):
        assert torch.equal(x, y)


def test_stream_block_one_byte_short_is_refused(engine):
    st, g = _stream_state(engine, "ff")
    lib, need = engine.lib, st.nbytes
    s = torch.cuda.current_stream().cuda_stream
    z64 = torch.zeros((R,), dtype=torch.int64, device="cuda")
    on = torch.ones((R,), dtype=torch.uint8, device="cuda")
    E = torch.zeros((3 * R, D), dtype=torch.float32, device="cuda")
    info = torch.zeros((R, 3, 4), dtype=torch.int32, device="cuda")
    cls = torch.zeros((R, 589), dtype=torch.uint8, device="cuda")
    cent = WC.sentinel_out((R, CAPACITY, D), torch.float32)
    counts = WC.sentinel_out((R, CAPACITY), torch.int32)
    K = WC.sentinel_out((R,), torch.int32)
    outs = (st.labels, st.score, st.K, st.emit_lo, st.emit_n, st.count, st.speakers)
    before = [t.clone() for t in outs]
    calls = {
        "sdk_stream_reset": lambda n: lib.sdk_stream_reset(engine.ctx, st.buf.data_ptr(), n, R, CAPACITY, D, None, s),
        "sdk_stream_step": lambda n: lib.sdk_stream_step(engine.ctx, E.data_ptr(), info.data_ptr(), cls.data_ptr(), z64.data_ptr(), on.data_ptr(), None, R, 589, D,
                                                         CAPACITY, HOP, LATENCY, 0.6, 2, st.buf.data_ptr(), n, *(t.data_ptr() for t in outs), s),
        "sdk_stream_flush": lambda n: lib.sdk_stream_flush(engine.ctx, z64.data_ptr(), on.data_ptr(), R, CAPACITY, D, 2, st.buf.data_ptr(), n,
                                                           *(t.data_ptr() for t in outs[3:]), s),
        "sdk_stream_centroids": lambda n: lib.sdk_stream_centroids(engine.ctx, st.buf.data_ptr(), n, R, CAPACITY, D, 0, R, cent.ptr, counts.ptr, K.ptr, None, s),
    }
    for entry, call in calls.items():
        rc = call(need - 1)
        msg = _err(engine)
        assert rc != 0, f"{entry}: a state block of {need - 1} bytes was accepted ({need} needed)"
        assert str(need - 1) in msg and str(need) in msg and entry in msg, (entry, msg)
    torch.cuda.synchronize()
    assert bool((st.buf == 0xFF).all()) and g.intact()
    assert all(torch.equal(a, b) for a, b in zip(before, outs))
    assert all((b.host() == WC.SENTINEL_BYTE).all() and b.tail_intact() for b in (cent, counts, K))
