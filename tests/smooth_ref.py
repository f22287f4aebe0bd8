"""The smoothing rule of smooth.py restated speaker by speaker in plain Python loops (no numpy in the rule itself), and the tables the CPU and
GPU tests of the smoothing share: hand-made edge cases, and seeded random tables with run structure (a random table of independent frames
has no gap worth filling and no run worth keeping).  Every case names what it is for and `holds` asserts, on the host, that it shows it."""
from __future__ import annotations

import numpy as np

T = 256                # smooth.SMOOTH_BLOCK_FRAMES: the frames one workgroup serves; the kernels stage no halo, they read across a workgroup's
HALO = T               # edges from memory, so the longest walk that stays within one neighbouring workgroup stands in for "the halo length"
MAX = 1024             # smooth.MAX_SMOOTH_FRAMES


def smooth_ref(speakers, frame_off, cent_off, fill, keep, cap):
    """-> (speakers [G, 2] int32, tallies [R, 2] int32, crowded): crowded = the frames with more fillers than free slots."""
    sp = np.asarray(speakers).reshape(-1, 2).tolist()
    out, tallies, crowded = [[-1, -1] for _ in sp], [], 0
    for r in range(len(frame_off) - 1):
        a, b, K = int(frame_off[r]), int(frame_off[r + 1]), int(cent_off[r + 1]) - int(cent_off[r])
        n = b - a
        inp = []
        for g in range(a, b):                                   # the speakers each frame names, in slot order, each once
            row = []
            for x in sp[g]:
                if 0 <= x < K and x not in row:
                    row.append(x)
            inp.append(row)
        everyone = sorted({k for row in inp for k in row})
        fillers = [[] for _ in range(n)]
        for k in everyone:                                      # 1 fill: between two consecutive frames of k, at most `fill` frames apart
            at = [g for g in range(n) if k in inp[g]]
            for p, q in zip(at[:-1], at[1:]):
                if 1 <= q - p - 1 <= fill:
                    for g in range(p + 1, q):
                        fillers[g].append(k)
        mid, filled = [], 0
        for g in range(n):                                      # 2 cap: the frame's own speakers, then its fillers in ascending k
            row = list(inp[g])
            crowded += len(fillers[g]) > max(cap - len(row), 0)
            for k in sorted(fillers[g]):
                if len(row) >= cap:
                    break
                row.append(k)
                filled += 1
            mid.append(row)
        res, dropped = [list(row) for row in mid], 0
        for k in everyone if keep > 0 else []:                  # 3 drop: every run of k shorter than keep
            g = 0
            while g < n:
                if k not in mid[g]:
                    g += 1
                    continue
                e = g
                while e < n and k in mid[e]:
                    e += 1
                if e - g < keep:
                    for f in range(g, e):
                        res[f].remove(k)
                        dropped += 1
                g = e
        for g in range(n):
            out[a + g] = (res[g] + [-1, -1])[:2]
        tallies.append([filled, dropped])
    return np.asarray(out, np.int32).reshape(-1, 2), np.asarray(tallies, np.int32).reshape(-1, 2), crowded


# ------------------------------------------------------------------------------------------------ tables
def run_table(rng, G: int, K: int, short: float = 0.5, noise: float = 0.03) -> np.ndarray:
    """[G, 2] int32 with run structure: each of up to 4 of the K speakers alternates runs and pauses whose lengths are short (1 .. 3 frames)
    with probability `short`, else 4 .. 40; a frame names up to two of its active speakers in a random slot order; `noise` of the entries
    become one of the forms that name nobody (-1, -7, K, K + 5) or repeat the other slot."""
    on = np.zeros((G, K), bool)
    for k in rng.choice(K, size=min(K, 4), replace=False):
        g, live = int(rng.integers(0, 6)), bool(rng.integers(0, 2))
        while g < G:
            n = int(rng.integers(1, 4)) if rng.random() < short else int(rng.integers(4, 41))
            on[g:g + n, k] = live
            g, live = g + n, not live
    sp = np.full((G, 2), -1, np.int32)
    for g in range(G):
        ks = np.nonzero(on[g])[0]
        ks = rng.permutation(ks)[:2]
        slots = rng.permutation(2)[:len(ks)]
        sp[g, slots] = ks
    hit = np.nonzero(rng.random((G, 2)) < noise)
    for g, s in zip(*hit):
        sp[g, s] = (-1, -7, K, K + 5, sp[g, 1 - s])[int(rng.integers(0, 5))]
    return sp


def pack(tables, Ks):
    """-> (speakers [G, 2], frame_off [R + 1], cent_off [R + 1])."""
    sp = np.concatenate([np.asarray(t, np.int32).reshape(-1, 2) for t in tables]) if tables else np.zeros((0, 2), np.int32)
    return sp, np.concatenate([[0], np.cumsum([len(t) for t in tables])]).astype(np.int64), np.concatenate([[0], np.cumsum(Ks)]).astype(np.int64)


def solo(pattern, k=0):
    """'#' names k, '.' is silent -> [G, 2]."""
    return np.asarray([[k, -1] if c == "#" else [-1, -1] for c in pattern], np.int32)


def gap_case(fill: int):
    """Speaker 0: 3 frames, a pause of exactly `fill` (filled), 2 frames, a pause of fill + 1 (not filled), 3 frames; the middle of the first
    pause lies on the edge of a workgroup.  Speaker 1 speaks through the first half of every pause, so the fillers take a second slot there."""
    edge = T * max(1, -(-(fill // 2 + 3) // T))
    start = edge - max(fill // 2, 1) - 3
    sp = solo("." * start + "###" + "." * fill + "##" + "." * (fill + 1) + "###" + "..")
    a, b = start + 3, start + 3 + fill + 2
    sp[a:a + fill // 2, 1] = 1
    sp[b:b + (fill + 1) // 2, 1] = 1
    return sp, (a, a + fill), (b, b + fill + 1)


def keep_case(keep: int):
    """Speaker 0: a run of keep - 1 frames (dropped) and a run of keep (kept), three silent frames between; the middle of the second run lies
    on the edge of a workgroup."""
    edge = T * -(-(keep // 2 + keep + 2) // T)
    start = edge - keep // 2 - keep - 2
    sp = solo("." * start + "#" * (keep - 1) + "..." + "#" * keep + "..")
    return sp, (start, start + keep - 1), (start + keep + 2, start + 2 * keep + 2)


def cases():
    """name -> dict(sp, frame_off, cent_off, fill, keep, cap, want): want holds the facts the case must show (checked by `holds`)."""
    rng = np.random.default_rng(20240)
    out = {}

    def add(name, tables, Ks, fill, keep, cap, **want):
        sp, fo, co = pack(tables, Ks)
        out[name] = dict(sp=sp, frame_off=fo, cent_off=co, fill=fill, keep=keep, cap=cap, want=want)

    # the sizes around a workgroup: one recording, three speakers
    add("G1", [[[0, 0]]], [3], 2, 2, 2, G=1, dropped=True)
    add("G2", [[[0, -1], [1, 0]]], [3], 2, 2, 2, G=2, dropped=True)
    for G in (T - 1, T, T + 1, 2 * T + 3):
        add(f"G{G}", [run_table(rng, G, 3)], [3], 2, 2, 2, G=G, filled=True, dropped=True)
    # packs: a boundary inside a workgroup, on its edge, an empty recording in the middle; at every boundary the last frames of one recording
    # and the first of the next would make a gap if the boundary were not there
    for name, lens in (("R3_inside", [100, 300, 150]), ("R3_edge", [T, T, 40]), ("R7_empty", [130, 126, 0, 300, 1, 2, 77])):
        Ks = [(1, 3, 40)[r % 3] for r in range(len(lens))]
        tables = [run_table(rng, n, K) for n, K in zip(lens, Ks)]
        for t in tables:
            if len(t) >= 4:
                t[:2], t[-2:] = [[-1, -1], [0, -1]], [[0, -1], [-1, -1]]
        add(name, tables, Ks, 4, 3, 2, filled=True, dropped=True, boundaries=True)
    # fill: a pause of exactly fill and one of fill + 1, astride the edge of the first workgroup
    for fill in (0, 1, 2, HALO, MAX):
        sp, yes, no = gap_case(fill)
        add(f"fill{fill}", [sp], [2], fill, 0, 2, filled=fill > 0, gap_filled=yes if fill else None, gap_open=no, astride=yes if fill > 1 else None)
    # keep: a run of keep - 1 and one of keep, astride the edge; longer than a whole recording; 0 and 1 drop nothing
    for keep in (2, HALO, MAX):
        sp, gone, stays = keep_case(keep)
        add(f"keep{keep}", [sp], [1], 0, keep, 2, dropped=True, run_gone=gone, run_stays=stays, astride=stays)
    add("keep_over_recording", [run_table(rng, 50, 3), run_table(rng, 60, 3)], [3, 3], 1, 61, 2, dropped=True, nothing_left=True)
    for keep in (0, 1):
        add(f"keep{keep}", [run_table(rng, T + 9, 3)], [3], 2, keep, 2, filled=True, dropped=False)
    # the cap: three speakers want frame 2; speaker 2 wants frames 1 and 3, which are full
    crowd = [[2, -1], [0, 1], [-1, -1], [0, 1], [2, -1]]
    add("crowd_cap2", [crowd], [3], 3, 0, 2, crowded=True, filled=True, out=[[2, -1], [0, 1], [0, 1], [0, 1], [2, -1]])
    add("crowd_cap1", [crowd], [3], 3, 0, 1, crowded=True, filled=True, out=[[2, -1], [0, 1], [0, -1], [0, 1], [2, -1]])
    for cap in (1, 2):
        add(f"cap{cap}_random", [run_table(rng, 2 * T + 3, 40, short=0.7), run_table(rng, T, 3, short=0.7)], [40, 3], 3, 2, cap, filled=True, dropped=True, crowded=True)
    add("K1", [run_table(rng, T + 40, 1)], [1], 1, 5, 2, filled=True, dropped=True)
    add("K40", [run_table(rng, T + 40, 40)], [40], 3, 3, 2, filled=True, dropped=True)
    return out


def random_pack(seed: int):
    rng = np.random.default_rng(seed)
    R = int(rng.integers(2, 8))
    lens = [int(rng.integers(0, 3 * T)) for _ in range(R)]
    Ks = [int(rng.choice([1, 3, 40])) for _ in range(R)]
    sp, fo, co = pack([run_table(rng, n, K) for n, K in zip(lens, Ks)], Ks)
    return dict(sp=sp, frame_off=fo, cent_off=co, fill=int(rng.integers(1, 9)), keep=int(rng.integers(2, 9)), cap=int(rng.integers(1, 3)),
                want=dict(filled=True, dropped=True))


def names(table):
    return [set(int(x) for x in row if x >= 0) for row in np.asarray(table).tolist()]


def holds(case, out, tallies, crowded):
    """Asserts that the case shows what it is for, given the reference's result for it."""
    w, sp, fo = case["want"], case["sp"], case["frame_off"]
    filled, dropped = int(tallies[:, 0].sum()), int(tallies[:, 1].sum())
    if "G" in w:
        assert len(sp) == w["G"]
    if "filled" in w:
        assert (filled > 0) == w["filled"], ("filled", filled)
    if "dropped" in w:
        assert (dropped > 0) == w["dropped"], ("dropped", dropped)
    if w.get("crowded"):
        assert crowded > 0
    if w.get("boundaries"):                                       # both sides of every boundary name 0 two frames apart, and the frames between stay silent
        hit = 0
        for b in fo[1:-1].tolist():
            if 2 <= b <= len(sp) - 2 and b - 2 >= 0 and sp[b - 2, 0] == 0 and sp[b + 1, 0] == 0 and (sp[b - 1:b + 1] < 0).all():
                assert case["fill"] >= 2 and not names(out[b - 1:b + 1])[0] and not names(out[b - 1:b + 1])[1]
                hit += 1
        assert hit >= 1
    if w.get("gap_filled"):
        a, b = w["gap_filled"]
        assert all(0 in s for s in names(out[a:b])) and not any(0 in s for s in names(sp[a:b]))
    if w.get("gap_open"):
        a, b = w["gap_open"]
        assert not any(0 in s for s in names(out[a:b])) and 0 in names(out[a - 1:a])[0] and 0 in names(out[b:b + 1])[0]
    if w.get("run_gone"):
        a, b = w["run_gone"]
        assert all(0 in s for s in names(sp[a:b])) and not any(0 in s for s in names(out[a:b]))
    if w.get("run_stays"):
        a, b = w["run_stays"]
        assert all(0 in s for s in names(out[a:b])) and 0 not in names(out[a - 1:a])[0] and 0 not in names(out[b:b + 1])[0]
    if w.get("astride"):
        a, b = w["astride"]
        assert a // T != (b - 1) // T                             # the stretch lies in more than one workgroup
    if w.get("nothing_left"):
        assert (out < 0).all() and case["keep"] > int(np.diff(fo).max())
    if "out" in w:
        assert out.tolist() == w["out"]
