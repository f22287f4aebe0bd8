"""tests/colstats_ref.py on the CPU: the reference against a per-row loop, the geometry classes of the shared shape table (every class of
the statistics epilogue must be reached - a later edit of the table cannot lose one), and the exactness conditions of the generated operands."""
import pytest
import torch

import colstats_ref as R


def _brute(A, Wt, Cin, taps, dil, T, bias, scale, shift, relu):
    """one output element at a time, plain Python floats"""
    M, N = A.shape[0], Wt.shape[0]
    out = [[0.0] * N for _ in range(M)]
    for m in range(M):
        b, t = divmod(m, T)
        for n in range(N):
            acc = 0.0
            for j in range(taps):
                u = t + (j - taps // 2) * dil
                u = -u if u < 0 else u
                u = 2 * (T - 1) - u if u >= T else u
                for c in range(Cin):
                    acc += float(A[b * T + u, c]) * float(Wt[n, j * Cin + c])
            acc += float(bias[n])
            if relu:
                acc = max(acc, 0.0)
            out[m][n] = acc * float(scale[n]) + float(shift[n])
    s = [[sum(out[b * T + t][n] for t in range(T)) for n in range(N)] for b in range(M // T)]
    q = [[sum(out[b * T + t][n] ** 2 for t in range(T)) for n in range(N)] for b in range(M // T)]
    return torch.tensor(out, dtype=torch.float64), torch.tensor(s, dtype=torch.float64), torch.tensor(q, dtype=torch.float64)


@pytest.mark.parametrize("T,B,N,Cin,taps,dil", [(5, 2, 4, 3, 3, 2), (4, 3, 3, 2, 1, 1)])
def test_reference_equals_a_per_row_loop(T, B, N, Cin, taps, dil):
    g = torch.Generator().manual_seed(T + taps)
    A = torch.randint(-2, 3, (T * B, Cin + 1), generator=g).float()          # a wider A: only the first Cin columns count
    Wt = torch.randint(-1, 2, (N, taps * Cin), generator=g).float()
    bias, shift = torch.randint(-3, 4, (N,), generator=g).float(), torch.randint(-2, 3, (N,), generator=g).float()
    scale = torch.tensor([0.5, 1.0, 2.0])[torch.arange(N) % 3]
    for fmt in ("bf16", "fp16"):
        ref = R.reference(A, Wt, Cin, taps, dil, T, bias, scale, shift, True, fmt)
        out, s, q = _brute(A, Wt, Cin, taps, dil, T, bias, scale, shift, True)
        assert torch.equal(ref.out, out) and torch.equal(ref.s, s) and torch.equal(ref.q, q)
        assert torch.equal(ref.mean, s / T)
        z = out.reshape(B, T, N)
        sd = ((z - z.mean(1, keepdim=True)) ** 2).mean(1).sqrt()
        assert torch.allclose(ref.std, sd, rtol=1e-12, atol=1e-12)
        assert R.exact_conditions(ref)[2]
    plain = R.reference(A, Wt, Cin, taps, dil, T, None, None, None, False, "bf16")
    assert torch.equal(plain.out, _brute(A, Wt, Cin, taps, dil, T, [0.0] * N, [1.0] * N, [0.0] * N, False)[0]) and plain.quantum == 1.0


def test_reference_refuses_values_the_format_cannot_hold():
    A = torch.full((4, 1), 3.0)
    Wt = torch.tensor([[1.0]])
    with pytest.raises(AssertionError):
        R.reference(A, Wt, 1, 1, 1, 4, torch.tensor([254.0]), None, None, False, "bf16")      # 257 needs nine significand bits
    assert R.reference(A, Wt, 1, 1, 1, 4, torch.tensor([254.0]), None, None, False, "fp16").s.item() == 4 * 257.0


def test_geometry_of_hand_worked_shapes():
    # M = 384, T = 128: tiles [0, 256) (segments 0, 1) and [256, 384) (segment 2; its lower half is outside); boundaries on half starts only
    assert R.geometry(384, 128) == {("nseg", 2), ("nseg", 1), ("outside", "lower")}
    # M = 800, T = 160: boundaries 160 (tile 0, lower half, wave 1), 320 (tile 1, upper, wave 2), 480 (tile 1, lower, wave 3), 640 (half start);
    # the last tile holds rows 768 ... 799: one wave inside, seven outside
    assert R.geometry(800, 160) == {("nseg", 2), ("nseg", 3), ("nseg", 1), ("wave_start", 1), ("wave_start", 2), ("wave_start", 3),
                                    ("outside", "upper"), ("outside", "lower")}
    # M = 274, T = 137: the boundary 137 is 9 rows into the wave at 128; the edge 274 is 18 rows into the wave at 256 (upper half)
    assert R.geometry(274, 137) == {("nseg", 2), ("nseg", 1), ("boundary", 9), ("edge", "gt16", "upper"), ("outside", "upper"), ("outside", "lower")}
    # M = 432, T = 144: edge 16 rows into the wave at 416 = tile 1, row 160 (lower half)
    assert ("edge", "eq16", "lower") in R.geometry(432, 144) and ("edge", "eq16", "upper") in R.geometry(528, 176)


def test_shape_table_reaches_every_class():
    hit = {}
    for T, B in R.SHAPES:
        for c in R.geometry(T * B, T):
            hit.setdefault(c, []).append((T, B))
    for c in sorted(R.ALL_CLASSES, key=str):
        print(c, "<-", hit.get(c, []))
    assert set(hit) <= R.ALL_CLASSES, set(hit) - R.ALL_CLASSES
    assert not R.ALL_CLASSES - set(hit), f"classes no shape reaches: {sorted(R.ALL_CLASSES - set(hit), key=str)}"
    assert len(R.ALL_CLASSES) == 3 + 31 + 3 + 6 + 2


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("T,B", R.SHAPES)
def test_generated_operands_meet_the_exactness_conditions(T, B, fmt):
    """N = 512 as the GPU cases use it: the stored values are exact in the format (asserted by reference()), every fp32 partial sum is exact,
    every ordinary column has variance >= 1 (the std bound's fixture condition) and the forced columns are all zero."""
    o, ref = R.case(T, B, 512, fmt=fmt)
    a, q, ok = R.exact_conditions(ref)
    print(f"T={T} B={B} {fmt}: quantum {ref.quantum}, max sum|v|/quantum {a:.0f}, max sum v^2/quantum^2 {q:.0f} (limit {2 ** 24}), "
          f"max |v| {float(ref.out.abs().max())}, min ordinary variance {float(_ordinary(ref.std, o['zero']).min()) ** 2:.3f}")
    assert ok
    assert float(_ordinary(ref.std, o["zero"]).min()) >= 1.0
    assert not ref.out[:, o["zero"]].any()
    assert o["A"].abs().max() <= 2 and o["Wt"].abs().max() <= 1 and set(o["scale"].tolist()) <= {0.5, 1.0, 2.0}


@pytest.mark.parametrize("T,B,N,taps,dil,fmts", [(129, 34, 512, 3, 2, ("bf16", "fp16")), (160, 5, 512, 3, 2, ("bf16", "fp16")),
                                                  (129, 34, 4096, 1, 1, ("bf16", "fp16")), (201, 200, 1024, 1, 1, ("bf16",))])
def test_operands_of_the_other_gpu_cases_meet_the_conditions(T, B, N, taps, dil, fmts):
    """the conv-tap cases, the persistent-reuse case and the half-tile-tail case of tests/test_conv_gemm_colstats_gpu.py"""
    for fmt in fmts:
        o, ref = R.case(T, B, N, taps=taps, dil=dil, fmt=fmt)
        a, q, ok = R.exact_conditions(ref)
        print(f"T={T} B={B} N={N} taps={taps} {fmt}: max sum|v|/quantum {a:.0f}, max sum v^2/quantum^2 {q:.0f}, max |v| {float(ref.out.abs().max())}, "
              f"min ordinary std {float(_ordinary(ref.std, o['zero']).min()):.3f}")
        assert ok and float(_ordinary(ref.std, o["zero"]).min()) >= 1.0 and not ref.out[:, o["zero"]].any()


def _ordinary(x, zero):
    keep = torch.ones(x.shape[1], dtype=torch.bool)
    keep[zero] = False
    return x[:, keep]
