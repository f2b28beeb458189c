"""fp32 GEMM on the bf16 matrix core (exact 3-way bf16 split, six products: csrc/split_bf16.h
`split3_bits` / `mfma_emu6`) against a float64 reference, side by side with the native
v_mfma_f32_32x32x2_f32 path. The emulated path must carry fp32 accuracy: its error, measured
against |A| @ |B| (the scale of the rounding error any fp32 summation order makes), stays within a
small multiple of the native f32 MFMA path's error and within an absolute fp32 bound."""
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24  # fp32 unit roundoff


@pytest.fixture(scope="module")
def C():
    from tutorial_torch_distributed_data_parallel_amd._native import native

    c = native()
    yield c
    c.gemm_f32_set_emu(True)


def _run(C, A, B, a_k, b_k, emu, **kw):
    M = A.shape[0] if a_k else A.shape[1]
    N = B.shape[0] if b_k else B.shape[1]
    out = torch.empty(M, N, device="cuda")
    C.gemm_f32_set_emu(emu)
    try:
        C.gemm_f32(A, B, out, a_k, b_k, **kw)
    finally:
        C.gemm_f32_set_emu(True)
    torch.cuda.synchronize()
    return out


def _scaled_err(out, A, B, a_k, b_k):
    A2 = (A if a_k else A.t()).double()
    B2 = (B.t() if b_k else B).double()
    ref = A2 @ B2
    scale = A2.abs() @ B2.abs()
    return ((out.double() - ref).abs() / scale.clamp_min(1e-30)).max().item()


SHAPES = [(128, 4096, 9216, True, True),    # toy-MLP fc1 forward (split-K)
          (128, 4096, 4096, True, False),   # fc2 input gradient
          (4096, 4096, 128, False, False),  # fc2 weight gradient (FN=2 tiles)
          (512, 384, 256, True, True),
          (130, 66, 257, True, True),       # ragged edges, K tail (257 % 32 != 0)
          (260, 136, 44, False, True),
          (64, 8, 4, True, True)]


@pytest.mark.parametrize("M,N,K,a_k,b_k", SHAPES)
@pytest.mark.parametrize("dist", ["normal", "wide"])
def test_emu_matches_fp64_like_native_f32(C, M, N, K, a_k, b_k, dist):
    torch.manual_seed(M * 7 + N * 3 + K)
    A = torch.randn((M, K) if a_k else (K, M), device="cuda")
    B = torch.randn((N, K) if b_k else (K, N), device="cuda")
    if dist == "wide":  # 2^[-20, 20] magnitudes: every split term is exercised, none underflows
        A = A * torch.exp2(torch.randint(-20, 21, A.shape, device="cuda").float())
        B = B * torch.exp2(torch.randint(-20, 21, B.shape, device="cuda").float())
    e_emu = _scaled_err(_run(C, A, B, a_k, b_k, True), A, B, a_k, b_k)
    e_nat = _scaled_err(_run(C, A, B, a_k, b_k, False), A, B, a_k, b_k)
    # fp32 summation of K products: worst case ~K*u, typical ~sqrt(K)*u; the six-term split
    # adds <= ~3u per product. Both paths must sit inside the fp32 bound.
    bound = (8 + 2 * K ** 0.5) * U
    assert e_nat < bound, (e_nat, bound)
    assert e_emu < bound, (e_emu, bound)
    assert e_emu < 4 * e_nat + 16 * U, (e_emu, e_nat)


def test_emu_split_is_exact_on_representable_products(C):
    # 12-bit A (split into hi + mid) times 6-bit B: 18-bit products, 32 of them sum to <= 23
    # bits, exact in fp32 -- the split path must reproduce them bit for bit
    g = torch.Generator(device="cpu").manual_seed(3)
    M = N = 64
    K = 32
    A = (torch.randint(-(2 ** 11), 2 ** 11, (M, K), generator=g).float() * 2.0 ** -5).cuda()
    B = (torch.randint(-(2 ** 5), 2 ** 5, (N, K), generator=g).float() * 2.0 ** -7).cuda()
    ref = (A.double() @ B.double().t()).float()
    out = _run(C, A, B, True, True, True)
    torch.testing.assert_close(out, ref, rtol=0, atol=0)


def test_emu_epilogues_and_identity(C):
    n = 64
    A = torch.eye(n, device="cuda")
    B = torch.randn(n, n, device="cuda")  # full-mantissa values survive the split exactly
    out = _run(C, A, B, True, False, True)
    torch.testing.assert_close(out, B, rtol=0, atol=0)
    x = torch.randn(256, 320, device="cuda")
    w = torch.randn(192, 320, device="cuda") / 18
    b = torch.randn(192, device="cuda")
    out = _run(C, x, w, True, True, True, bias=b, relu=True)
    ref = torch.relu(x.double() @ w.double().t() + b.double()).float()
    torch.testing.assert_close(out, ref, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("emu", [True, False])
def test_conv_paths_under_both_products(emu):
    # implicit-GEMM forward / input-gradient / weight-gradient kernels share the split path
    import torch.nn.functional as F

    from tutorial_torch_distributed_data_parallel_amd import ops
    from tutorial_torch_distributed_data_parallel_amd._native import native

    Cn = native()
    Cn.gemm_f32_set_emu(emu)
    try:
        torch.manual_seed(5)
        x = torch.randn(4, 64, 14, 14, device="cuda", requires_grad=True)
        w = (torch.randn(128, 64, 3, 3, device="cuda") / 24).requires_grad_()
        y = ops.conv2d(x, w, None, 1, 1)
        dy = torch.randn_like(y)
        y.backward(dy)
        torch.cuda.synchronize()
    finally:
        Cn.gemm_f32_set_emu(True)
    xr = x.detach().double().cpu().requires_grad_()
    wr = w.detach().double().cpu().requires_grad_()
    yr = F.conv2d(xr, wr, None, 1, 1)
    yr.backward(dy.double().cpu())
    torch.testing.assert_close(y.double().cpu(), yr, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(x.grad.double().cpu(), xr.grad, rtol=1e-5, atol=1e-4)
    torch.testing.assert_close(w.grad.double().cpu(), wr.grad, rtol=1e-5, atol=1e-4)


@pytest.mark.parametrize("ea,eb", [(-100, 90), (110, -100), (-20, -60)])
def test_emu_extreme_exponents(C, ea, eb):
    """Operands around 2^ea and 2^eb (products normal): every split term of the small operand is
    itself a normal fp32 number down to ~2^-110, so the six-product sum keeps fp32 accuracy;
    checked against fp64 next to the native f32 MFMA path."""
    torch.manual_seed(abs(ea) * 31 + abs(eb))
    M, N, K = 130, 96, 160
    A = torch.randn(M, K, device="cuda") * 2.0 ** ea
    B = torch.randn(N, K, device="cuda") * 2.0 ** eb
    e_emu = _scaled_err(_run(C, A, B, True, True, True), A, B, True, True)
    e_nat = _scaled_err(_run(C, A, B, True, True, False), A, B, True, True)
    bound = (8 + 2 * K ** 0.5) * U
    assert e_nat < bound and e_emu < bound, (e_emu, e_nat, bound)


def test_emu_subnormal_operands_documented_bound(C):
    """Operands at the bottom of the fp32 range (2^-128 .. 2^-126, subnormal or barely normal)
    times ~2^+118: their lower split terms are bf16 subnormals that the bf16 path flushes, so the
    split path's error relative to |A| @ |B| grows to ~2^-8 there (the native f32 MFMA keeps
    fp32 accuracy). Pinned bound, documented in docs/PARITY.md; operands above ~2^-110 keep
    fp32 accuracy (test_emu_extreme_exponents)."""
    torch.manual_seed(9)
    M, N, K = 64, 64, 64
    A = torch.randn(M, K, device="cuda") * 2.0 ** -128
    A[:, ::2] *= 4.0  # half the columns normal (2^-126), half subnormal
    B = torch.randn(N, K, device="cuda") * 2.0 ** 118
    emu = _run(C, A, B, True, True, True)
    nat = _run(C, A, B, True, True, False)
    assert torch.isfinite(emu).all() and torch.isfinite(nat).all()
    e_emu = _scaled_err(emu, A, B, True, True)
    e_nat = _scaled_err(nat, A, B, True, True)
    assert e_nat < (8 + 2 * K ** 0.5) * U, e_nat
    assert e_emu < 2.0 ** -6, e_emu


def test_emu_non_finite_inputs_stay_non_finite(C):
    """inf / NaN operands: the split path turns inf into NaN (x - bf16(x) = inf - inf), so the
    pinned contract is finiteness: an output is finite exactly when the native f32 MFMA's is.
    Finite operands up to 3e38 (below bf16's 3.39e38 maximum) stay finite and accurate; above
    3.39e38 the bf16 head term overflows (documented in docs/PARITY.md)."""
    torch.manual_seed(4)
    M, N, K = 64, 64, 64
    A = torch.randn(M, K, device="cuda")
    B = torch.randn(N, K, device="cuda")
    A[3, 5] = float("inf")
    A[7, 1] = float("-inf")
    A[9, 2] = float("nan")
    B[11, 5] = 0.0  # inf * 0 = NaN in both paths
    emu = _run(C, A, B, True, True, True)
    nat = _run(C, A, B, True, True, False)
    assert torch.equal(torch.isfinite(emu), torch.isfinite(nat))
    assert not torch.isfinite(emu[3]).any() and not torch.isfinite(emu[9]).any()
    big = (torch.rand(M, K, device="cuda") * 2 - 1) * 3.0e38  # |x| <= 3e38 < bf16 max 3.39e38
    small = torch.randn(N, K, device="cuda") * 1e-12
    out = _run(C, big, small, True, True, True)
    assert torch.isfinite(out).all(), (big.abs().max().item(), (~torch.isfinite(out)).sum().item())
    e_emu = _scaled_err(out, big, small, True, True)
    assert e_emu < (8 + 2 * K ** 0.5) * U, e_emu



@pytest.mark.parametrize("bk", [True, False])
def test_gemm_f32_dispatches_large_plain_gemms_to_emu8(bk):
    """gemm_f32 on a large plain GEMM (>= 256 256x256 tiles in whole waves) runs the 256 x 256
    kernel (csrc/gemm_emu8.hip): bias + ReLU epilogue, bitwise equal to the 128 x 128 fast
    kernel (same six products in the same k order), within the fp32 bound against fp64."""
    import torch

    from tutorial_torch_distributed_data_parallel_amd._native import native

    C = native()
    torch.manual_seed(11)
    M, N, K = 4096, 4096, 1024
    A = torch.randn(M, K, device="cuda")
    B = torch.randn((N, K) if bk else (K, N), device="cuda")
    bias = torch.randn(N, device="cuda")
    auto = torch.empty(M, N, device="cuda")
    fast = torch.empty(M, N, device="cuda")
    direct = torch.empty(M, N, device="cuda")
    C.gemm_f32(A, B, auto, True, bk, bias=bias, relu=True)
    C.gemm_f32_set_mode(2)
    try:
        C.gemm_f32(A, B, fast, True, bk, bias=bias, relu=True)
    finally:
        C.gemm_f32_set_mode(0)
    C.gemm_emu8(A, B, direct, bk)
    torch.cuda.synchronize()
    assert torch.equal(auto, fast)
    assert torch.equal(auto, torch.relu(direct + bias))
    Bm = B.t() if bk else B
    rows = torch.randperm(M, device="cuda")[:128]
    ref = torch.relu(A[rows].double() @ Bm.double() + bias.double())
    torch.testing.assert_close(auto[rows].double(), ref, rtol=1e-4, atol=1e-3)
