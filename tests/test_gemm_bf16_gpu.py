"""Mixed-precision GEMM (csrc/gemm_bf16.hip): fp32 tensors, every operand element rounded once to
bf16 (RNE), one bf16 MFMA product per K16 step, fp32 accumulation.

The oracle is float64 on the ROUNDED operands. bf16 x bf16 products are exact in fp32, so the only
error is the fp32 accumulation: scaled by |bf(A)| @ |bf(B)| it stays under (8 + 2 sqrt(K)) 2^-24,
the bound tests/test_gemm_emu_gpu.py uses for the same MFMA instruction."""
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
KK, KM, MM = (True, True), (True, False), (False, False)  # (a_kcontig, b_kcontig)


@pytest.fixture(scope="module")
def C():
    from tutorial_torch_distributed_data_parallel_amd._native import native

    return native()


def _bound(K):
    return (8 + 2 * K ** 0.5) * U


def _operands(M, N, K, a_k, b_k, dist="normal", seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed + M * 7 + N * 3 + K)
    A = torch.randn((M, K) if a_k else (K, M), generator=g)
    B = torch.randn((N, K) if b_k else (K, N), generator=g)
    if dist == "wide":  # 2^[-20, 20] magnitudes
        A = A * torch.exp2(torch.randint(-20, 21, A.shape, generator=g).float())
        B = B * torch.exp2(torch.randint(-20, 21, B.shape, generator=g).float())
    return A.cuda(), B.cuda()


def _oracle(A, B, a_k, b_k):
    """(float64 product of the bf16-rounded operands, its |.| @ |.| scale)"""
    A2 = (A if a_k else A.t()).bfloat16().double()
    B2 = (B.t() if b_k else B).bfloat16().double()
    return A2 @ B2, A2.abs() @ B2.abs()


def _scaled_err(out, ref, scale):
    return ((out.double() - ref).abs() / scale.clamp_min(1e-300)).max().item()


def _run(C, A, B, a_k, b_k, **kw):
    M = A.shape[0] if a_k else A.shape[1]
    N = B.shape[0] if b_k else B.shape[1]
    out = kw.pop("out", None)
    if out is None:
        out = torch.empty(M, N, device="cuda")
    C.gemm_bf16(A, B, out, a_k, b_k, **kw)
    torch.cuda.synchronize()
    return out


CASES = [(64, 8, 4, KK), (64, 8, 4, KM), (64, 8, 4, MM),
         (130, 66, 257, KK), (130, 66, 257, KM), (130, 66, 257, MM),  # ragged, K tail, unaligned
         (260, 136, 44, MM),                                          # weight-gradient layout
         (128, 10, 512, KK),                                          # head: N < one tile
         (32, 256, 4608, KK),                                         # skinny M, long K: split-K
         (512, 384, 256, KK), (512, 384, 256, KM), (512, 384, 256, MM)]


@pytest.mark.parametrize("M,N,K,lay", CASES)
@pytest.mark.parametrize("dist", ["normal", "wide"])
def test_matches_rounded_operand_oracle(C, M, N, K, lay, dist):
    a_k, b_k = lay
    A, B = _operands(M, N, K, a_k, b_k, dist)
    out = _run(C, A, B, a_k, b_k)
    ref, scale = _oracle(A, B, a_k, b_k)
    e = _scaled_err(out, ref, scale)
    print(f"scaled error {e / U:.2f} u, bound {_bound(K) / U:.2f} u")
    assert e < _bound(K), (e, _bound(K))


def test_plan_paths(C):
    """The skinny shape takes split-K; ragged / unaligned shapes the guarded loads; aligned
    multiples of the tile depth the vector loads."""
    def plan(M, N, K, a_k, b_k):
        A, B = _operands(M, N, K, a_k, b_k)
        return C.gemm_bf16_plan(A, B, torch.empty(M, N, device="cuda"), a_k, b_k)

    splits, kps, guarded = plan(32, 256, 4608, True, True)
    assert splits > 1 and kps % 64 == 0 and splits * kps >= 4608 and not guarded
    assert plan(130, 66, 257, True, True)[2] == 1
    assert plan(260, 136, 44, False, False)[2] == 1
    assert plan(512, 384, 256, False, False)[2] == 0
    assert plan(512, 384, 256, True, False)[2] == 0
    assert plan(4096, 4096, 128, False, False)[0] == 1  # enough tiles: no split


@pytest.mark.parametrize("lay", [KK, KM, MM])
def test_exact_on_representable_operands(C, lay):
    # 8-bit integers times a power of two are bf16 values; 32 products of <= 16 bits sum below
    # 2^24 in units of the common scale: every partial sum is exact in fp32, in any order
    a_k, b_k = lay
    g = torch.Generator(device="cpu").manual_seed(5)
    M, N, K = 96, 80, 32
    A = (torch.randint(-255, 256, (M, K) if a_k else (K, M), generator=g).float() * 2.0 ** -5).cuda()
    B = (torch.randint(-255, 256, (N, K) if b_k else (K, N), generator=g).float() * 2.0 ** 3).cuda()
    ref = ((A if a_k else A.t()).double() @ (B.t() if b_k else B).double()).float()
    out = _run(C, A, B, a_k, b_k)
    assert torch.equal(out, ref)


def test_operands_are_really_rounded(C):
    M, N, K = 128, 128, 256
    A, B = _operands(M, N, K, True, True)  # randn: full 24-bit significands
    out = _run(C, A, B, True, True)
    ref, scale = _oracle(A, B, True, True)
    assert _scaled_err(out, ref, scale) < _bound(K)
    f32 = torch.empty(M, N, device="cuda")
    C.gemm_f32(A, B, f32, True, True)
    torch.cuda.synchronize()
    # against the fp32 GEMM the operand rounding (2^-9 relative per operand) shows
    assert _scaled_err(out, f32.double(), scale) > _bound(K)


def test_bias_relu_epilogue(C):
    M, N, K = 130, 66, 257
    A, B = _operands(M, N, K, True, True)
    bias = torch.randn(N, device="cuda")
    out = _run(C, A, B, True, True, bias=bias, relu=True)
    ref, scale = _oracle(A, B, True, True)
    want = (ref + bias.double()).clamp_min(0)
    # the bias add is one more fp32 rounding of the sum
    err = (out.double() - want).abs()
    assert (err <= _bound(K) * scale + U * want.abs()).all()
    assert (out >= 0).all() and (out == 0).any()


@pytest.mark.parametrize("M,N,K", [(130, 66, 257), (128, 256, 128)])
def test_gate_epilogue(C, M, N, K):
    A, B = _operands(M, N, K, True, False)
    gate = torch.randn(M, N, device="cuda")
    plain = _run(C, A, B, True, False)
    gated = _run(C, A, B, True, False, gate=gate)
    assert torch.equal(gated, torch.where(gate > 0, plain, torch.zeros_like(plain)))


@pytest.mark.parametrize("M,N,K,lay", [(130, 66, 257, KK), (32, 256, 4608, KK)])
def test_beta_one_accumulates(C, M, N, K, lay):
    a_k, b_k = lay
    A, B = _operands(M, N, K, a_k, b_k)
    c0 = torch.randn(M, N, device="cuda")
    plain = _run(C, A, B, a_k, b_k)
    acc = _run(C, A, B, a_k, b_k, out=c0.clone(), beta=1.0)
    assert torch.equal(acc, plain + c0)
    with pytest.raises(RuntimeError):
        C.gemm_bf16(A, B, c0, a_k, b_k, beta=0.5)


@pytest.mark.parametrize("M,N,K", [(260, 136, 44), (512, 384, 256)])
def test_rowsum_is_the_unrounded_batch_sum(C, M, N, K):
    g, x = _operands(M, N, K, False, False)  # g [K = batch][M = out], x [K][N = in]
    db = torch.empty(M, device="cuda")
    _run(C, g, x, False, False, rowsum=db)
    want = g.double().sum(0)
    # fp32 summation of K terms, any order: <= K u sum|g|
    assert ((db.double() - want).abs() <= K * U * g.double().abs().sum(0)).all()
    # and not the sum of the rounded values
    assert not torch.equal(db, g.bfloat16().float().sum(0))
    # K-contiguous A: the row sums of A itself
    A, B = _operands(M, N, K, True, True)
    rs = torch.empty(M, device="cuda")
    _run(C, A, B, True, True, rowsum=rs)
    assert ((rs.double() - A.double().sum(1)).abs() <= K * U * A.double().abs().sum(1)).all()


@pytest.mark.parametrize("M,N,K,lay", [(130, 66, 257, KM), (32, 256, 4608, KK),
                                         (512, 384, 256, MM)])
def test_bitwise_reproducible(C, M, N, K, lay):
    a_k, b_k = lay
    A, B = _operands(M, N, K, a_k, b_k)
    assert torch.equal(_run(C, A, B, a_k, b_k), _run(C, A, B, a_k, b_k))


@pytest.mark.parametrize("lay", [KK, MM])
def test_non_finite_operands(C, lay):
    a_k, b_k = lay
    M, N, K = 64, 48, 128
    A, B = _operands(M, N, K, a_k, b_k)
    if a_k:
        A[3, 5] = float("inf")
    else:
        A[5, 3] = float("inf")
    if b_k:
        B[7, 9] = float("nan")
    else:
        B[9, 7] = float("nan")
    out = _run(C, A, B, a_k, b_k)
    ref, _ = _oracle(A, B, a_k, b_k)
    ref = ref.float()
    assert torch.equal(out.isnan(), ref.isnan())
    assert torch.equal(out.isinf(), ref.isinf())
    assert torch.equal(out[out.isinf()], ref[ref.isinf()])
    assert out.isnan().any() and out.isinf().any()


def test_strided_views_and_refusals(C):
    # row strides that are no multiple of 4 floats and an unaligned base: the guarded loads
    big = torch.randn(70, 201, device="cuda")
    A = big[1:66, 3:103]           # [65][100], stride 201, base offset 4-B aligned only
    Bw = torch.randn(40, 131, device="cuda")[:, 1:101]
    out = torch.empty(65, 44, device="cuda")[:, :40]
    C.gemm_bf16(A, Bw, out, True, True)
    torch.cuda.synchronize()
    ref, scale = _oracle(A, Bw, True, True)
    assert _scaled_err(out, ref, scale) < _bound(100)
    with pytest.raises(RuntimeError):
        C.gemm_bf16(A.double(), Bw, out, True, True)
    with pytest.raises(RuntimeError):
        C.gemm_bf16(A, Bw[:, :50], out, True, True)
