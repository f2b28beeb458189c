"""CPU self-tests of tests/gemm_oracle.py: the checker accepts a correct fp32 result (torch on the
CPU) at the shapes tests/test_gemm_f32_matrix_gpu.py uses and rejects each of the kernel mistakes
that file is there to catch; the input conditions (share of closed gate / mask / ReLU elements,
the five special values inside the last ragged tile) hold for every shape."""
import pytest
import torch

import gemm_oracle as O

# (M, N, K) of the GPU file: fast / 256-row / generic / skinny / emu8 cases
SHAPES = [(132, 68, 160), (132, 68, 44), (260, 196, 260), (132, 66, 160), (260, 67, 260),
          (37, 68, 44), (77, 13, 260), (33, 64, 16), (16, 100, 300), (260, 262, 64)]
EPI = dict(beta=0.5, relu=True)


def _epilogue(P, prod, *, bias=True, beta=0.5, relu=True, gate=True, C0=None):
    """fp32 epilogue in the kernels' order on an fp32 product."""
    C = prod.clone()
    if bias:
        C = C + P.bias
    if beta:
        C = C + beta * (P.C0 if C0 is None else C0)
    if relu:
        C = torch.relu(C)
    if gate:
        C = torch.where(O.closed(P.gate), torch.zeros_like(C), C)
    return C


def _ref(P, **kw):
    args = dict(bias=P.bias, beta=0.5, C0=P.C0, relu=True, gate=P.gate)
    args.update(kw)
    return O.reference(P.A, P.B, True, False, **args)


def _rejects(fn, *a, **kw):
    with pytest.raises(AssertionError):
        fn(*a, **kw)


@pytest.fixture(scope="module")
def P():
    return O.Problem(132, 68, 160, seed=1)


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_good_output_passes_and_inputs_meet_their_conditions(M, N, K):
    P = O.Problem(M, N, K, seed=2)
    O.has_specials(P.gate)
    O.has_specials(P.mask)
    r0, c0 = O.ragged_corner(M, N)
    assert all(r >= r0 and c >= c0 for r, c in O.special_slots(M, N))
    r = O.reference(P.A, P.B, True, False, mask=P.mask, bias=P.bias, beta=0.5, C0=P.C0,
                    relu=True, gate=P.gate, rowsum_beta=0.5, rowsum0=P.rowsum0)
    for what in ("mask", "relu", "gate"):  # asserted inside reference(); shown here
        assert 0.25 <= r.shares[what] <= 0.75, (what, r.shares[what])
    good, rs = O.torch_f32(P.A, P.B, True, False, mask=P.mask, bias=P.bias, beta=0.5, C0=P.C0,
                           relu=True, gate=P.gate, rowsum_beta=0.5, rowsum0=P.rowsum0)
    f = O.framed(M, N, fill="pattern")
    f.view.copy_(good)
    O.frame_intact(f)
    # the good output also stands in for torch's: e_k = e_t, any c >= 0 passes
    O.check_ref(f.view, r, t32=good, c=0)
    O.check_rowsum(rs, r, t32=rs, c=0)
    # other storage of the same operands gives the same reference
    r2 = O.reference(P.A.t().contiguous(), P.B.t().contiguous(), False, True,
                     mask=P.mask.t().contiguous(), bias=P.bias, beta=0.5, C0=P.C0, relu=True,
                     gate=P.gate, rowsum_beta=0.5, rowsum0=P.rowsum0)
    assert O.scaled_err(r2[0], r[0], r[2]) < 2.0 ** -45  # float64 summation order only
    assert O.scaled_err(r2[1], r[1], r.rowsum_scale) < 2.0 ** -45
    assert torch.equal(r.must_zero, r2.must_zero)


def test_share_conditions_are_enforced():
    P = O.Problem(132, 68, 160, seed=3)
    _rejects(O.reference, P.A, P.B, True, False, gate=P.gate.abs() + 1.0)      # nothing closed
    _rejects(O.reference, P.A, P.B, True, False, mask=-P.mask.abs())           # all closed
    _rejects(O.reference, P.A, P.B, True, False, bias=P.bias + 1e4, relu=True)  # nothing zeroed
    _rejects(O.has_specials, torch.randn(132, 68))
    g = P.gate.clone()
    r, c = O.special_slots(132, 68)[4]
    g[0, 0], g[r, c] = g[r, c].item(), 1.0  # the subnormal moved out of the ragged tile
    _rejects(O.has_specials, g)


def test_rejects_dropped_k_index_in_one_tile(P):
    r = _ref(P)
    prod = P.A @ P.B
    O.check_ref(_epilogue(P, prod), r)
    prod[:128, 64:] -= P.A[:128, 37:38] @ P.B[37:38, 64:]
    _rejects(O.check_ref, _epilogue(P, prod), r)


def test_rejects_missing_bias_in_last_column_group(P):
    r = _ref(P)
    C = torch.relu(P.A @ P.B + torch.cat([P.bias[:64], torch.zeros(4)]) + 0.5 * P.C0)
    C = torch.where(O.closed(P.gate), torch.zeros_like(C), C)
    _rejects(O.check_ref, C, r)


def test_rejects_swapped_columns_in_last_tile(P):
    r = _ref(P)
    prod = P.A @ P.B
    prod[:, [64, 65]] = prod[:, [65, 64]]
    _rejects(O.check_ref, _epilogue(P, prod), r)
    # and bitwise on the selection input
    A = O.selection(P.M, P.K)
    want = P.B[O.selection_rows(P.M, P.K)]
    got = A @ P.B
    assert torch.equal(got, want)
    got[:, [64, 65]] = got[:, [65, 64]]
    assert not torch.equal(got, want)


def test_rejects_gate_ge_zero_and_nan_gate(P):
    r = _ref(P)
    pre = torch.relu(P.A @ P.B + P.bias + 0.5 * P.C0)
    good = torch.where(O.closed(P.gate), torch.zeros_like(pre), pre)
    O.check_ref(good, r)
    ge = torch.where(P.gate >= 0, pre, torch.zeros_like(pre))  # opens 0.0 and -0.0
    assert (ge != good).sum().item() == 2
    _rejects(O.check_ref, ge, r)
    nan_open = torch.where(P.gate <= 0, torch.zeros_like(pre), pre)  # NaN <= 0 is false: open
    assert (nan_open != good).sum().item() == 1
    _rejects(O.check_ref, nan_open, r)


def test_rejects_beta_applied_twice(P):
    r = _ref(P)
    _rejects(O.check_ref, _epilogue(P, P.A @ P.B + 0.5 * P.C0), r)


def test_rejects_relu_before_bias(P):
    r = _ref(P)
    C = torch.relu(P.A @ P.B + 0.5 * P.C0) + P.bias
    _rejects(O.check_ref, torch.where(O.closed(P.gate), torch.zeros_like(C), C), r)


@pytest.mark.parametrize("M,N,K", [(132, 68, 44), (132, 68, 160), (260, 196, 260)])
def test_rejects_dropped_third_split_term(M, N, K):
    """bf16 split without its third term = A rounded to 16 significand bits. On N(0, 1) data the
    errors average out below the absolute bound; on the wide distribution a few products carry
    each sum and the 2^-17 relative error shows, against the absolute bound and against torch."""
    P = O.Problem(M, N, K, seed=4, dist="wide")
    r = O.reference(P.A, P.B, True, False)
    good = P.A @ P.B
    O.check_ref(good, r, t32=good, c=4)
    bits = P.A.view(torch.int32)
    A16 = ((bits + 0x80) & ~0xFF).view(torch.float32)
    bad = A16 @ P.B
    _rejects(O.check_ref, bad, r)
    with pytest.raises(AssertionError, match="4 \\*"):
        # the relative rule alone rejects it as well (bound made vacuous: K -> very large)
        O.check(bad, r[0], r[2], 10 ** 9, t32=good, c=4)


def test_rejects_writes_outside_the_window_and_unwritten_elements(P):
    r = _ref(P)
    good = _epilogue(P, P.A @ P.B)
    for fill in (float("nan"), "pattern"):
        for spot in ("right", "below", "above"):
            f = O.framed(P.M, P.N, fill=fill)
            f.view.copy_(good)
            O.frame_intact(f)
            r0, r1, c0, c1 = f.window
            where = {"right": (r0 + 3, c1), "below": (r1, c0 + 5), "above": (r0 - 1, c1 - 1)}[spot]
            f.buf[where] = 0.0
            _rejects(O.frame_intact, f)
        f = O.framed(P.M, P.N, fill=fill)
        keep = f.view[130, 66].item()
        f.view.copy_(good)
        f.view[130, 66] = keep  # one interior element never written
        O.frame_intact(f)
        _rejects(O.check_ref, f.view, r)
    v = O.framed_vec(P.M)
    v.view.zero_()
    O.frame_intact(v)
    v.buf[v.window[1]] = 1.0
    _rejects(O.frame_intact, v)


def test_frames_are_aligned_and_strided():
    f = O.framed(132, 68, ld_extra=8)
    assert f.view.stride() == (76, 1) and f.view.data_ptr() % 16 == 0
    f = O.framed(132, 66, ld_extra=8)
    assert f.view.stride() == (74, 1) and f.view.data_ptr() % 16 == 0
    f = O.framed(132, 68, pad_cols=1, ld_extra=8)
    assert f.view.data_ptr() % 16 == 4
    a = O.strided(torch.randn(37, 44), ld_extra=1, offset=1)
    assert a.stride() == (45, 1) and a.data_ptr() % 16 == 4


def test_rejects_rowsum_of_unmasked_a():
    P = O.Problem(132, 68, 160, seed=5, a_mean=100.0)
    r = O.reference(P.A, P.B, True, False, mask=P.mask, rowsum_beta=0.5, rowsum0=P.rowsum0)
    Am = torch.where(O.closed(P.mask), torch.zeros_like(P.A), P.A)
    O.check_rowsum(Am.sum(1) + 0.5 * P.rowsum0, r)
    _rejects(O.check_rowsum, P.A.sum(1) + 0.5 * P.rowsum0, r)
    # mean 100, spread 1: a rowsum of the wrong rows (shifted by one tile row) loses visibly
    _rejects(O.check_rowsum, torch.roll(Am.sum(1), 1) + 0.5 * P.rowsum0, r)
