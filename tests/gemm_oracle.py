"""Float64 oracle of the fp32 GEMM family (csrc/gemm_f32.hip, gemm_f32_fast.hip, gemm_skinny.hip,
gemm_emu8.hip), the project's tolerance rule on the scaled error, and sentinel frames.

A helper for tests/test_gemm_oracle_cpu.py and tests/test_gemm_f32_matrix_gpu.py, not a test.
Plain torch: nothing here needs a GPU, every function works on whatever device its inputs are on.

Semantics (csrc/kernels.h, GemmF32Args), on LOGICAL operands A [M, K] and B [K, N] whatever their
storage:

    A'      = A where mask > 0, else 0          (NaN, -0.0, 0 and negatives close the mask)
    C       = A' . B + bias + beta * C0
    C       = max(C, 0)                         (relu)
    C       = C where gate > 0, else 0          (the same rule as the mask)
    rowsum  = rowsum_beta * rowsum0 + sum_k A'  (unrounded A')

Tolerance (``check``). The rounding error of any fp32 summation order of sum_k a_k b_k is
proportional to sum_k |a_k b_k|, so errors are measured relative to

    scale = |A'| . |B| + |bias| + |beta * C0|   (elementwise; rowsum: sum_k |A'| + |rb * rowsum0|)

as ``_scaled_err`` of tests/test_gemm_emu_gpu.py does: e = max |got - ref| / scale.
  * e_k < (8 + 2 sqrt(K)) * 2^-24: the bound test_gemm_emu_gpu.py and the grouped-convolution
    tests use (typical fp32 summation error ~ sqrt(K) u, the six-product split <= ~3 u more);
  * with a torch fp32 result t32 of the same problem: e_k <= 4 e_t + c * 2^-24
    (tests/test_hard_inputs_gpu.py: 4 allows for another summation order, c is recorded per
    quantity by the caller).
Elements the reference sets to zero are not compared by tolerance: where the gate is closed, or
where ReLU zeroes a pre-activation that is negative by more than the absolute bound (its sign is
then beyond any rounding), the output must be +0.0 or -0.0 exactly. A pre-activation within the
bound of zero may legitimately come out on either side and is compared by tolerance against 0."""
import math

import torch

U = 2.0 ** -24  # fp32 unit roundoff


def abs_bound(K):
    """The project's absolute bound on the scaled error of a K-term fp32 dot product."""
    return (8 + 2 * math.sqrt(K)) * U


class Ref(tuple):
    """(C_ref, rowsum_ref, scale) with, as attributes, what ``check`` needs beyond them:
    ``must_zero`` (bool, C's shape), ``rowsum_scale`` and the measured input shares."""


def closed(t):
    """Where a gate / mask element closes: !(t > 0)."""
    return ~(t > 0)


def reference(A, B, a_k=True, b_k=True, *, mask=None, bias=None, beta=0.0, C0=None, relu=False,
              gate=None, rowsum_beta=0.0, rowsum0=None, want_rowsum=False, shares=True):
    """Float64 reference from the fp32 inputs. A is stored [M, K] if a_k else [K, M]; B [N, K] if
    b_k else [K, N]; mask in A's storage; C0 and gate [M, N]. Returns Ref(C, rowsum, scale).

    With ``shares`` the input conditions of the test plan are asserted: a gate, a mask and a ReLU
    each close between 25 % and 75 % of their elements."""
    A2 = (A if a_k else A.t()).double()
    B2 = (B.t() if b_k else B).double()
    K = A2.shape[1]
    info = {}
    if mask is not None:
        mc = closed(mask if a_k else mask.t())
        A2 = torch.where(mc, torch.zeros_like(A2), A2)
        info["mask"] = mc.double().mean().item()
    pre = A2 @ B2
    scale = A2.abs() @ B2.abs()
    if bias is not None:
        pre = pre + bias.double()
        scale = scale + bias.double().abs()
    beta = float(torch.tensor(beta, dtype=torch.float32))  # the kernels hold beta as float
    if beta != 0.0:
        pre = pre + beta * C0.double()
        scale = scale + (beta * C0.double()).abs()
    C = pre
    must_zero = torch.zeros_like(pre, dtype=torch.bool)
    if relu:
        C = C.clamp_min(0.0)
        must_zero |= pre < -abs_bound(K) * scale
        info["relu"] = (pre < 0).double().mean().item()
    if gate is not None:
        gc = closed(gate)
        C = torch.where(gc, torch.zeros_like(C), C)
        must_zero |= gc
        info["gate"] = gc.double().mean().item()
    rowsum = rowsum_scale = None
    if want_rowsum or rowsum0 is not None:
        rowsum = A2.sum(1)
        rowsum_scale = A2.abs().sum(1)
        rb = float(torch.tensor(rowsum_beta, dtype=torch.float32))
        if rb != 0.0:
            rowsum = rowsum + rb * rowsum0.double()
            rowsum_scale = rowsum_scale + (rb * rowsum0.double()).abs()
    if shares:
        for what, share in info.items():
            assert 0.25 <= share <= 0.75, f"{what} closes {share:.1%} of its elements"
    out = Ref((C, rowsum, scale))
    out.must_zero = must_zero
    out.rowsum_scale = rowsum_scale
    out.shares = info
    out.K = K
    return out


def scaled_err(got, ref, scale, skip=None):
    """max |got - ref| / scale over the elements not in ``skip``; NaN if any of them is NaN."""
    d = (got.double() - ref).abs() / scale.clamp_min(1e-300)
    if skip is not None:
        d = torch.where(skip, torch.zeros_like(d), d)
    if d.numel() == 0:
        return 0.0
    return float("nan") if torch.isnan(d).any() else d.max().item()


def check(got, ref, scale, K, t32=None, c=None, must_zero=None, what="C"):
    """Assert the tolerance rule for one output; prints the figures first. Returns (e_k, e_t)."""
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} != {tuple(ref.shape)}"
    assert got.dtype == torch.float32, f"{what}: dtype {got.dtype}"
    if must_zero is not None and must_zero.any():
        z = got[must_zero]
        nz = int((z != 0).sum().item())  # NaN != 0 too
        assert nz == 0, f"{what}: {nz} of {z.numel()} gated / rectified elements are not +-0.0"
    e_k = scaled_err(got, ref, scale, must_zero)
    bound = abs_bound(K)
    e_t = None
    if t32 is not None:
        e_t = scaled_err(t32, ref, scale, must_zero)
    print(f"[gemm] {what}: e_k={e_k / U:.2f}u" + (f" e_t={e_t / U:.2f}u" if e_t is not None else "")
          + f" bound={bound / U:.1f}u" + (f" c={c} need={(e_k - 4 * e_t) / U:.2f}"
                                           if e_t is not None else ""))
    assert e_k < bound, f"{what}: e_k {e_k / U:.2f} u >= (8 + 2 sqrt({K})) = {bound / U:.1f} u"
    if t32 is not None:
        assert e_k <= 4 * e_t + c * U, \
            f"{what}: e_k {e_k / U:.2f} u > 4 * {e_t / U:.2f} u + {c} u"
    return e_k, e_t


def check_ref(got, r, t32=None, c=None, what="C"):
    """``check`` of a C output against a ``reference`` result."""
    return check(got, r[0], r[2], r.K, t32=t32, c=c, must_zero=r.must_zero, what=what)


def check_rowsum(got, r, t32=None, c=None, what="rowsum"):
    return check(got, r[1], r.rowsum_scale, r.K, t32=t32, c=c, what=what)


def torch_f32(A, B, a_k=True, b_k=True, *, mask=None, bias=None, beta=0.0, C0=None, relu=False,
              gate=None, rowsum_beta=0.0, rowsum0=None):
    """The same operation by torch in fp32 (torch.matmul + a torch epilogue): the e_t side of the
    rule. Returns (C, rowsum)."""
    A2 = A if a_k else A.t()
    B2 = B.t() if b_k else B
    if mask is not None:
        A2 = torch.where(closed(mask if a_k else mask.t()), torch.zeros_like(A2), A2)
    C = A2 @ B2
    if bias is not None:
        C = C + bias
    if beta != 0.0:
        C = C + beta * C0
    if relu:
        C = torch.relu(C)
    if gate is not None:
        C = torch.where(closed(gate), torch.zeros_like(C), C)
    rs = A2.sum(1)
    if rowsum_beta != 0.0:
        rs = rs + rowsum_beta * rowsum0
    return C, rs


# ------------------------------------------------------------------------------------- frames
class Frame:
    """An output window inside a larger sentinel-filled buffer (see ``framed``)."""

    def __init__(self, buf, sentinel, window):
        self.buf, self.sentinel, self.window = buf, sentinel, window

    @property
    def view(self):
        r0, r1, c0, c1 = self.window
        return self.buf[r0:r1, c0:c1] if self.buf.dim() == 2 else self.buf[r0:r1]


def _pattern(shape, device):
    """The fixed finite sentinel: distinct-looking values nothing in a test produces."""
    n = 1
    for s in shape:
        n *= s
    i = torch.arange(n, dtype=torch.int64)
    return (-(7.0e4 + ((i * 37) % 1021).double())).float().reshape(shape).to(device)


def framed(M, N, pad_rows=8, pad_cols=0, ld_extra=8, fill=float("nan"), device="cpu",
           rows_below=8):
    """An [M, N] view inside a [pad_rows + M + rows_below, pad_cols + N + ld_extra] buffer filled
    with the sentinel: ``fill`` = NaN (beta == 0 calls) or "pattern", a fixed finite pattern
    (beta != 0 calls: write C0 into ``.view`` first). The view's leading dimension is
    pad_cols + N + ld_extra; its first element is 16-byte aligned when pad_cols % 4 == 0 (the rows
    above it are pad_rows = 8 whole rows). Every call into the view is a valid call: the frame
    only makes a store past row M / column N of a ragged tile visible."""
    assert rows_below >= 8 and ld_extra >= 8, "frames keep >= 8 rows / columns of margin"
    assert pad_rows % 4 == 0
    shape = (pad_rows + M + rows_below, pad_cols + N + ld_extra)
    if isinstance(fill, str):
        buf = _pattern(shape, device)
    else:
        buf = torch.full(shape, fill, dtype=torch.float32, device=device)
    f = Frame(buf, buf.clone(), (pad_rows, pad_rows + M, pad_cols, pad_cols + N))
    if pad_cols % 4 == 0:
        assert f.view.data_ptr() % 16 == 0
    return f


def framed_vec(M, pad=8, fill=float("nan"), device="cpu"):
    """The 1-D form (a rowsum): a contiguous [M] view with ``pad`` sentinels on either side."""
    assert pad >= 8 and pad % 4 == 0
    shape = (pad + M + pad,)
    if isinstance(fill, str):
        buf = _pattern(shape, device)
    else:
        buf = torch.full(shape, fill, dtype=torch.float32, device=device)
    return Frame(buf, buf.clone(), (pad, pad + M, 0, 0))


def frame_intact(f):
    """Assert that every element outside the window still holds its sentinel bit for bit."""
    same = f.buf.view(torch.int32) == f.sentinel.view(torch.int32)
    r0, r1, c0, c1 = f.window
    if f.buf.dim() == 2:
        same[r0:r1, c0:c1] = True
    else:
        same[r0:r1] = True
    bad = (~same).nonzero()
    assert bad.numel() == 0, \
        f"{bad.shape[0]} elements outside the window {f.window} were overwritten, first at " \
        f"{bad[0].tolist()}"


def strided(t, ld_extra=0, offset=0):
    """A copy of the 2-D tensor t as a view with leading dimension cols + ld_extra whose first
    element sits ``offset`` floats into a 16-byte aligned allocation (offset 1: misaligned)."""
    R, Cc = t.shape
    ld = Cc + ld_extra
    buf = torch.zeros(offset + R * ld + 4, dtype=t.dtype, device=t.device)
    v = buf[offset:offset + R * ld].view(R, ld)[:, :Cc]
    v.copy_(t)
    return v


# ------------------------------------------------------------------------------------- inputs
SPECIALS = ("zero", "negzero", "nan", "negative", "subnormal")
_SPECIAL_VALUES = (0.0, -0.0, float("nan"), -1.5, 2.0 ** -140)
_TILES = (32, 64, 128, 256)


def ragged_corner(R, Cc):
    """(r0, c0): rows >= r0 and columns >= c0 lie in the last, ragged tile of an [R, Cc] matrix
    for every tile size the kernels use (the smallest nonzero remainder per axis)."""
    def rem(n):
        rs = [n % t for t in _TILES if n % t]
        return min(rs) if rs else _TILES[0]  # a multiple of every tile: its last 32
    return R - rem(R), Cc - rem(Cc)


def special_slots(R, Cc):
    """Where ``plant_specials`` puts the five values, in the order of SPECIALS."""
    r0, c0 = ragged_corner(R, Cc)
    slots = [(r, c) for r in range(r0, R) for c in range(c0, Cc)]
    assert len(slots) >= len(_SPECIAL_VALUES), f"ragged corner of {R}x{Cc} holds {len(slots)}"
    step = len(slots) // len(_SPECIAL_VALUES)
    return [slots[i * step] for i in range(len(_SPECIAL_VALUES))]


def plant_specials(t):
    """Overwrite five elements of the last ragged tile of the [R, Cc] gate / mask t with 0.0,
    -0.0, NaN, a negative value and a positive subnormal (in place); returns t."""
    for (r, c), v in zip(special_slots(*t.shape), _SPECIAL_VALUES):
        t[r, c] = v
    return t


def has_specials(t):
    """Assert the five special values sit inside the last ragged tile of t."""
    R, Cc = t.shape
    r0, c0 = ragged_corner(R, Cc)
    corner = t[r0:, c0:].detach().cpu().reshape(-1)
    bits = corner.view(torch.int32)
    found = {
        "zero": bool((bits == 0).any()),
        "negzero": bool((bits == -(2 ** 31)).any()),
        "nan": bool(torch.isnan(corner).any()),
        "negative": bool((corner < 0).any()),
        "subnormal": bool(((corner > 0) & (corner < 2.0 ** -126)).any()),
    }
    missing = [k for k in SPECIALS if not found[k]]
    assert not missing, f"gate / mask lacks {missing} in its last ragged tile"


def gate_like(R, Cc, gen, device="cpu"):
    """A random gate / mask (about half closed) carrying the five special values."""
    return plant_specials(torch.randn(R, Cc, generator=gen)).to(device)


def wide(t, gen):
    """The 2^[-20, 20] magnitude spread of test_emu_matches_fp64_like_native_f32: a few products
    dominate every sum, so every term of the bf16 split matters."""
    return t * torch.exp2(torch.randint(-20, 21, t.shape, generator=gen).float())


def selection(M, K):
    """A [M, K] with a single 1.0 per row at column (7 m + 3) mod K: A . B = B[(7m+3) mod K, :]
    bit for bit on every path (a product by 1.0 and sums with zeros are exact)."""
    A = torch.zeros(M, K)
    m = torch.arange(M)
    A[m, (7 * m + 3) % K] = 1.0
    return A


def selection_rows(M, K):
    return (7 * torch.arange(M) + 3) % K


class Problem:
    """One logical GEMM problem on the CPU: A [M, K], B [K, N] and a full epilogue's inputs."""

    def __init__(self, M, N, K, seed=0, dist="normal", a_mean=0.0):
        g = torch.Generator().manual_seed(seed * 1000003 + M * 7919 + N * 101 + K)
        self.M, self.N, self.K = M, N, K
        self.A = torch.randn(M, K, generator=g) + a_mean
        self.B = torch.randn(K, N, generator=g)
        if dist == "wide":
            self.A, self.B = wide(self.A, g), wide(self.B, g)
        # |bias| and |C0| a visible share of the product's sqrt(K) magnitude
        s = math.sqrt(K)
        self.bias = torch.randn(N, generator=g) * s / 2
        self.C0 = torch.randn(M, N, generator=g) * s
        self.gate = plant_specials(torch.randn(M, N, generator=g))
        self.mask = plant_specials(torch.randn(M, K, generator=g))
        # under the special gate values the pre-activation is positive beyond doubt (beta * C0
        # = 8 sqrt(K) against a product of spread sqrt(K)), so a ReLU cannot hide a gate that
        # lets 0.0, -0.0 or NaN through
        for r, c in special_slots(M, N):
            self.C0[r, c] = 16 * s
        self.rowsum0 = torch.randn(M, generator=g) * s
        has_specials(self.gate)
        has_specials(self.mask)

    def to(self, device):
        for k, v in list(vars(self).items()):
            if torch.is_tensor(v):
                setattr(self, k, v.to(device))
        return self
