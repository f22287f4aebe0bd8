"""Test-side checker of the diarization pipeline (diarize.py, csrc/diarize.hip, the masked pooling of csrc/resnet.hip): the stated rules in
loop form, written from the rules and sharing no code with diarize.py.

  decode / masks / reconstruct   plain Python loops over frames, columns and chunks (reconstruct scans EVERY chunk per global frame)
  last_map / weighted_embed      resnet_ref.layer_boundary_embed's layer loop restated up to the pooling (that function does not return the
                                 last map), then the weighted statistics and seg_1 in float64
  *_fp32_in_order / *_one_pass   fp32 restatements of the poolings: the yardstick of their bounds, and the one-pass form the bounds must reject
  pool_case / pool_cases         the seeded inputs of the pooling edge tests (tests/test_diarize_edges_cpu.py, tests/test_diarize_edges_gpu.py)
  cluster / assign / order / turns / rttm   the host stages, with scipy's centroid linkage and ahc_ref's threshold rule
"""
from __future__ import annotations

import functools
import os
import sys
from typing import Optional

import numpy as np
import torch
import torch.nn.functional as Fn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resnet_ref as RR  # noqa: E402
from ahc_ref import threshold_rule  # noqa: E402

HOP, RATE, CHUNK, F_CHUNK = 270, 16000, 160000, 589
CLASSES = [set(), {0}, {1}, {2}, {0, 1}, {0, 2}, {1, 2}]
MIN_CLEAN, MIN_VALID, TRAIN_DEN = 4, 2, 5


# ------------------------------------------------------------------------------------------------------------ rules (a), (b), (d)
def decode(logp) -> np.ndarray:
    logp = np.asarray(logp)
    out = np.zeros(logp.shape[:-1], np.uint8)
    for idx in np.ndindex(*logp.shape[:-1]):
        best = 0
        for c in range(1, 7):
            if logp[idx][c] > logp[idx][best]:
                best = c
        out[idx] = best
    return out


def masks(cls, T4: int):
    B, F = cls.shape
    w = np.zeros((B, 3, T4), np.float32)
    info = np.zeros((B, 3, 4), np.int32)
    for b in range(B):
        for s in range(3):
            active = sum(1 for i in range(F) if s in CLASSES[cls[b, i]])
            clean_frames = sum(1 for i in range(F) if s in CLASSES[cls[b, i]] and len(CLASSES[cls[b, i]]) < 2)
            full, clean = [], []
            for j in range(T4):
                i = min(F - 1, (j * F) // T4)
                a = s in CLASSES[cls[b, i]]
                full.append(a)
                clean.append(a and len(CLASSES[cls[b, i]]) < 2)
            used = sum(clean) >= MIN_CLEAN
            row = clean if used else full
            w[b, s] = row
            info[b, s] = (active, clean_frames, used, sum(row) >= MIN_VALID)
    return w, info


def column_counts(cls, T4: int) -> np.ndarray:
    """-> [B, 3, 2] int: per (chunk, speaker) the columns of the last map in which the speaker is active, and those in which it is alone
    (the sums that masks() compares with MIN_CLEAN and MIN_VALID)."""
    B, F = cls.shape
    out = np.zeros((B, 3, 2), np.int64)
    for b in range(B):
        for j in range(T4):
            members = CLASSES[cls[b, min(F - 1, (j * F) // T4)]]
            for s in members:
                out[b, s, 0] += 1
                out[b, s, 1] += len(members) < 2
    return out


def n_global(n_samples: int) -> int:
    return max(0, (n_samples - 495 + 269) // 270)


def reconstruct(cls, starts, labels, K: int, n_samples: int, max_speakers: Optional[int] = None):
    """-> (count [G] uint8, speakers [G, 2] int32, act [G, K] int32, nc [G])."""
    C, F = cls.shape
    G = n_global(n_samples)
    count, speakers = np.zeros(G, np.uint8), np.full((G, 2), -1, np.int32)
    act, ncs = np.zeros((G, K), np.int32), np.zeros(G, np.int64)
    q = [(135 - int(starts[c])) // 270 for c in range(C)]
    for g in range(G):
        nc = cnt = 0
        for c in range(C):
            i = g + q[c]
            if not 0 <= i < F:
                continue
            nc += 1
            cnt += len(CLASSES[cls[c, i]])
            for k in {int(labels[c, s]) for s in CLASSES[cls[c, i]] if 0 <= labels[c, s] < K}:    # a label at or above K names no cluster
                act[g, k] += 1
        ncs[g] = nc
        if nc == 0:
            continue
        n = min((2 * cnt + nc) // (2 * nc), 2)
        if max_speakers is not None:
            n = min(n, max_speakers)
        count[g] = n
        ranked = sorted((k for k in range(K) if act[g, k] > 0), key=lambda k: (-act[g, k], k))
        for slot, k in enumerate(ranked[:n]):
            speakers[g, slot] = k
    return count, speakers, act, ncs


# ------------------------------------------------------------------------------------------------------------ embedding
def last_map(weights, feats: torch.Tensor, bits, blocks=(3, 4, 6, 3), acc=torch.float64) -> torch.Tensor:
    """resnet_ref.layer_boundary_embed's layer loop up to the pooling: feats [B, T, F] -> the last map [B, C, F4, T4]."""
    def conv(x, conv_name, bn_name, stride, pad):
        wf, shift = RR._fold(weights, conv_name, bn_name, acc)
        if bits is not None:
            wf = RR.round_bits(wf.to(torch.float32), bits)
        return Fn.conv2d(x, wf.to(acc), None, stride, pad), shift

    def f32(shift):
        return shift.to(torch.float32).to(acc) if bits is not None else shift.to(acc)

    x = feats.to(acc).transpose(1, 2).unsqueeze(1)
    y, b = conv(x, "conv1", "bn1", 1, 1)
    x = RR.round_bits(torch.relu(y + f32(b)[:, None, None]), bits)
    for l, nb in enumerate(blocks):
        for j in range(nb):
            p = f"layer{l + 1}.{j}"
            s = 2 if (j == 0 and l > 0) else 1
            y, b = conv(x, f"{p}.conv1", f"{p}.bn1", s, 1)
            h = RR.round_bits(torch.relu(y + f32(b)[:, None, None]), bits)
            y, b = conv(h, f"{p}.conv2", f"{p}.bn2", 1, 1)
            if f"{p}.shortcut.0.weight" in weights:
                ys, bs = conv(x, f"{p}.shortcut.0", f"{p}.shortcut.1", s, 0)
                y, b = y + ys, b + bs
                res = 0
            else:
                res = x
            x = RR.round_bits(torch.relu(y + f32(b)[:, None, None] + res), bits)
    return x


def weighted_stats(last: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """last [B, C, F4, T4], w [B, S, T4] -> float64 statistics [B, S, 2 C F4] (feature c F4 + f): the stated weighted mean | std."""
    x = last.double().reshape(last.shape[0], 1, -1, last.shape[-1])       # [B, 1, C F4, T4]
    w = w.double()[:, :, None, :]                                          # [B, S, 1, T4]
    v1, v2 = w.sum(-1), (w * w).sum(-1)
    mean = (w * x).sum(-1) / v1
    var = (w * (x - mean[..., None]) ** 2).sum(-1) / (v1 - v2 / v1)
    return torch.cat([mean, torch.sqrt(var + 1e-7)], dim=2)


def weighted_stats_fp32_in_order(last: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """The same statistic in fp32 with the kernel's summation order (frames in order, fused multiply-adds emulated by float64 products
    rounded once): the deviation of this from float64 is the yardstick of the pooling bound."""
    x = last.float().reshape(last.shape[0], 1, -1, last.shape[-1])
    w = w.float()[:, :, None, :]
    T = x.shape[-1]

    def fma(a, b, c):
        return (a.double() * b.double() + c.double()).float()
    v1 = torch.zeros(w.shape[:-1])
    v2 = torch.zeros(w.shape[:-1])
    for t in range(T):
        v1 = v1 + w[..., t]
        v2 = fma(w[..., t], w[..., t], v2)
    s = torch.zeros(w.shape[0], w.shape[1], x.shape[2])
    for t in range(T):
        s = fma(w[..., t].expand_as(s), x[..., t].expand_as(s), s)
    mean = s / v1
    q = torch.zeros_like(s)
    for t in range(T):
        d = x[..., t] - mean
        q = fma(w[..., t] * d, d, q)
    return torch.cat([mean, torch.sqrt(q / (v1 - v2 / v1) + 1e-7)], dim=2)


def weighted_stats_fp32_one_pass(last: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """What the pooling must NOT be: the same statistic in fp32 from ONE sweep (sum w x and sum w x^2 by fused multiply-adds in frame order,
    var = (sum w x^2 - (sum w x)^2 / v1) / (v1 - v2 / v1)).  On data with a large mean the subtraction cancels; the edge tests measure how
    far beyond the yardstick this lands, to show that their bound tells the two apart."""
    x = last.float().reshape(last.shape[0], 1, -1, last.shape[-1])
    w = w.float()[:, :, None, :]

    def fma(a, b, c):
        return (a.double() * b.double() + c.double()).float()
    v1 = torch.zeros(w.shape[:-1])
    v2 = torch.zeros(w.shape[:-1])
    s = torch.zeros(w.shape[0], w.shape[1], x.shape[2])
    q = torch.zeros_like(s)
    for t in range(x.shape[-1]):
        v1 = v1 + w[..., t]
        v2 = fma(w[..., t], w[..., t], v2)
        s = fma(w[..., t].expand_as(s), x[..., t].expand_as(s), s)
        q = fma(w[..., t] * x[..., t], x[..., t].expand_as(s), q)
    var = (q - s * s / v1) / (v1 - v2 / v1)
    return torch.cat([s / v1, torch.sqrt(var.clamp_min(0.0) + 1e-7)], dim=2)


def tstp_stats_fp32_in_order(x: torch.Tensor) -> torch.Tensor:
    """The unweighted pooling (resnet_ref.tstp_stats) in fp32 with the kernel's order on the channel-last map x [B, F, T, C] -> [B, 2 C F]:
    the sum in frame order, mean = s * (1 / T), the square sum by fused multiply-adds, q * (1 / (T - 1)), sqrt(. + 1e-7).  Its deviation
    from float64 is the yardstick of the unmasked pooling's bound."""
    B, F, T, C = x.shape
    x = x.float().permute(0, 3, 1, 2).reshape(B, C * F, T)
    s = torch.zeros(B, C * F)
    one = torch.ones_like(s)                                             # every constant as an fp32 tensor: no scalar is applied in a wider type
    inv_t, inv_t1, eps = one / torch.full_like(s, T), one / torch.full_like(s, T - 1), torch.full_like(s, 1e-7)
    for t in range(T):
        s = s + x[..., t]
    mean = s * inv_t
    q = torch.zeros_like(s)
    for t in range(T):
        d = x[..., t] - mean
        q = (d.double() * d.double() + q.double()).float()
    return torch.cat([mean, torch.sqrt(q * inv_t1 + eps)], dim=1)


# the edge shapes of the masked pooling (B, F4, T4, C, S): idle lanes (C < 256), the strided channel loop (C = 300, 512), a full speaker group
# (S = 4), a second group of one speaker (S = 5, 9), S T4 at the 12288-float LDS limit, and the production shape
POOL_SHAPES = [(1, 1, 2, 64, 1), (2, 3, 3, 32, 4), (2, 2, 37, 300, 5), (1, 2, 126, 512, 9), (1, 1, 4096, 64, 3), (3, 10, 126, 256, 3)]
# the unmasked pooling (B, F4, T4, C)
TSTP_SHAPES = [(1, 1, 2, 64), (2, 3, 9, 32), (2, 2, 37, 300), (1, 10, 126, 256), (1, 1, 1001, 512)]
POOL_DTYPE = {0: torch.bfloat16, 2: torch.float16}


def pool_data(rng, shape, data: str, fmt: int) -> torch.Tensor:
    """A channel-last last map in the 2-byte format fmt.  signed: randn; offset: 100 + 0.25 randn, rounded to the format (bf16 keeps steps
    of 0.5 there, fp16 of 1 / 16: a mean 200 to 1600 times the spread, which a one-pass variance does not survive in fp32)."""
    g = rng.standard_normal(shape).astype(np.float32)
    return torch.from_numpy(g if data == "signed" else 100.0 + 0.25 * g).to(POOL_DTYPE[fmt])


def pool_case(shape, data: str, weights: str, fmt: int):
    """Seeded inputs of one masked-pooling edge case -> (x [B, F4, T4, C] 2-byte, w [B, S, T4] fp32, valid [B, S] int32).
    binary weights: p = 0.4 with the first and the last column forced to 1 (every row has its two columns), and the middle column of
    row 0 of segment 0; fractional: uniform in [0.05, 1].  S >= 4: valid is mixed - row 1 of every segment is invalid with all-zero weights, row 3 invalid with weights, and in a second
    segment row 0 (zero weights) as well, so that valid is read at b S + s."""
    B, F4, T4, Cc, S = shape
    rng = np.random.default_rng([B, F4, T4, Cc, S, fmt, data == "offset", weights == "binary"])
    x = pool_data(rng, (B, F4, T4, Cc), data, fmt)
    if weights == "binary":
        w = (rng.random((B, S, T4)) < 0.4).astype(np.float32)
        w[:, :, 0] = w[:, :, -1] = 1.0
        w[0, 0, T4 // 2] = 1.0                                            # a valid row of three columns even at T4 = 3 (two columns divide exactly)
    else:
        w = (0.05 + 0.95 * rng.random((B, S, T4))).astype(np.float32)
    valid = np.ones((B, S), np.int32)
    if S >= 4:
        valid[:, 1] = valid[:, 3] = 0
        w[:, 1] = 0.0
        if B > 1:
            valid[1, 0] = 0
            w[1, 0] = 0.0
    return x, torch.from_numpy(w), torch.from_numpy(valid)


@functools.lru_cache(maxsize=None)
def pool_reference(shape, data: str, weights: str, fmt: int):
    """One edge case with its float64 statistics and its yardstick, computed once per process and left unchanged by its users ->
    (x, w, valid, want [B, S, 2 C F4] float64, yardstick: the fp32-in-order restatement's largest deviation over the valid rows)."""
    x, w, valid = pool_case(shape, data, weights, fmt)
    last = x.float().permute(0, 3, 1, 2)
    want = weighted_stats(last, w)
    ok = valid.bool()
    yard = float((weighted_stats_fp32_in_order(last, w).double() - want)[ok].abs().max())
    return x, w, valid, want, yard


@functools.lru_cache(maxsize=None)
def tstp_reference(shape, data: str, fmt: int):
    """One edge case of the unmasked pooling -> (x [B, F4, T4, C] 2-byte, want [B, 2 C F4] float64, yardstick)."""
    rng = np.random.default_rng(list(shape) + [fmt, data == "offset"])
    x = pool_data(rng, shape, data, fmt)
    want = RR.tstp_stats(x.float())
    return x, want, float((tstp_stats_fp32_in_order(x).double() - want).abs().max())


def pool_cases():
    """Every (shape, data, weights) of the edge tests; fractional weights from T4 = 37 on."""
    return [(sh, data, wk) for sh in POOL_SHAPES for data in ("signed", "offset") for wk in ("binary", "fractional") if wk == "binary" or sh[2] >= 37]


def weighted_embed(weights, last: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """-> raw embeddings [B, S, embed_dim] float64."""
    acc = torch.float64
    return weighted_stats(last, w) @ RR._t(weights, "seg_1.weight", acc).T + RR._t(weights, "seg_1.bias", acc)


# ------------------------------------------------------------------------------------------------------------ host stages
def training(info, F: int):
    rows = []
    flat = np.asarray(info).reshape(-1, 4)
    for r in range(flat.shape[0]):
        if flat[r, 3] and TRAIN_DEN * int(flat[r, 1]) >= F:
            rows.append(r)
    return rows


def cluster_training(E_train: np.ndarray, threshold: float, min_cluster_size: int):
    """-> (labels, Z): scipy's centroid linkage and the threshold rule of cluster.agglomerative_cluster."""
    from scipy.cluster.hierarchy import linkage
    n = E_train.shape[0]
    if n == 0:
        return np.zeros(0, np.int32), np.zeros((0, 4))
    if n == 1:
        return np.zeros(1, np.int32), np.zeros((0, 4))
    Z = linkage(np.asarray(E_train, np.float64), "centroid")
    return threshold_rule(Z, np.asarray(E_train, np.float64), threshold, min_cluster_size), Z


def assign(E, info, train_rows, train_labels):
    """-> (labels [C, 3], centroids [K, d] float64 unit, margins: best - second cosine of every assigned row (inf with one centroid))."""
    E = np.asarray(E, np.float64)
    flat = np.asarray(info).reshape(-1, 4)
    n = flat.shape[0]
    labels = np.full(n, -1, np.int32)
    cand = [r for r in range(n) if flat[r, 3] and flat[r, 0] > 0]
    if len(train_rows):
        K = int(max(train_labels)) + 1
        cent = []
        for k in range(K):
            rows = [r for r, lab in zip(train_rows, train_labels) if lab == k]
            m = np.zeros(E.shape[1])
            for r in rows:
                m = m + E[r]
            cent.append(m / len(rows))
    elif cand:
        m = np.zeros(E.shape[1])
        for r in cand:
            m = m + E[r]
        cent = [m / len(cand)]
    else:
        return labels.reshape(-1, 3), np.zeros((0, E.shape[1])), []
    cent = np.stack([c / np.linalg.norm(c) for c in cent])
    margins = []
    for r in cand:
        cos = [float(E[r] @ c) for c in cent]
        best = 0
        for k in range(1, len(cos)):
            if cos[k] > cos[best]:
                best = k
        labels[r] = best
        others = [cos[k] for k in range(len(cos)) if k != best]
        margins.append(cos[best] - max(others) if others else np.inf)
    return labels.reshape(-1, 3), cent, margins


def order_by_appearance(speakers, K: int):
    """new id per provisional cluster: first appearance in frame order, then slot order; clusters never seen follow in their old order."""
    seen = []
    for g in range(speakers.shape[0]):
        for slot in range(2):
            k = int(speakers[g, slot])
            if k >= 0 and k not in seen:
                seen.append(k)
    seen += [k for k in range(K) if k not in seen]
    new = [0] * K
    for i, k in enumerate(seen):
        new[k] = i
    return new


def turns(speakers, K: int):
    out = []
    G = speakers.shape[0]
    for k in range(K):
        g = 0
        while g < G:
            if k in speakers[g]:
                g1 = g
                while g1 + 1 < G and k in speakers[g1 + 1]:
                    g1 += 1
                out.append(((270 * g + 360) / 16000, (270 * g1 + 630) / 16000, k))
                g = g1 + 1
            else:
                g += 1
    return sorted(out, key=lambda t: (t[0], t[2]))


def rttm(turn_list, uri: str) -> str:
    lines = []
    for a, b, k in turn_list:
        lines.append("SPEAKER %s 1 %.3f %.3f <NA> <NA> SPEAKER_%02d <NA> <NA>\n" % (uri, a, b - a, k))
    return "".join(lines)


def stitch(cls, starts, labels, K: int, n_samples: int, max_speakers=None):
    """Provisional reconstruction, renumbering by appearance, final reconstruction -> (labels, order, count, speakers, turns)."""
    count, speakers, _, _ = reconstruct(cls, starts, labels, max(K, 1), n_samples, max_speakers)
    new = order_by_appearance(speakers, K)
    if K > 1 and new != list(range(K)):
        labels = np.array([[new[v] if v >= 0 else -1 for v in row] for row in labels], np.int32)
        count, speakers, _, _ = reconstruct(cls, starts, labels, K, n_samples, max_speakers)
    return labels, new, count, speakers, turns(speakers, K)


def pipeline(cls, starts, E, info, n_samples: int, threshold: float, min_cluster_size: int, max_speakers=None):
    """The host side of Diarizer.run on given class tables, unit embeddings E [C * 3, d] and info -> dict."""
    F = cls.shape[1]
    tr = training(info, F)
    tl, Z = cluster_training(np.asarray(E, np.float64)[tr], threshold, min_cluster_size)
    labels, cent, margins = assign(E, info, tr, tl)
    K = cent.shape[0]
    labels, new, count, speakers, tn = stitch(cls, starts, labels, K, n_samples, max_speakers)
    cent = cent[np.argsort(new)] if K else cent
    return dict(train=tr, train_labels=tl, Z=Z, labels=labels, centroids=cent, margins=margins, count=count, speakers=speakers, turns=tn, K=K)
