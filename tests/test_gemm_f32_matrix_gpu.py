"""Every plan and epilogue of the fp32 GEMM family against float64 at ragged shapes.

Each case pins the kernel it means to test: it reads ``gemm_f32_plan_for`` for the very tensors
(layouts, strides, alignment) it is about to pass and asserts the plan BEFORE it looks at numbers,
so a planner change fails loudly instead of moving the case onto another kernel. Outputs are
windows of sentinel-filled buffers (tests/gemm_oracle.py ``framed``): an element the kernel did not
write, a beta == 0 path that reads C, or a store past row M / column N of a ragged tile shows.
Numbers are judged by the oracle's rule on the scaled error: e_k < (8 + 2 sqrt(K)) u absolutely and
e_k <= 4 e_t + c u against torch's own fp32 result, u = 2^-24; gated / rectified elements must be
+-0.0 exactly; the selection-matrix input must come out bit for bit.

Shapes are the smallest with an edge for each mechanism (tiles 128 or 256 x 64 FN, K step 32):
M 132 / 260 (4 ragged rows, two 128- or 256-row tiles), N 68 / 196 (ragged against 64 and 128) and
66 / 67 for the scalar stores, K 44 / 160 / 260 (tails of 12 and 4). Two exceptions, by the
planner's own thresholds: the generic 128 x 128 tile needs M, N >= 512, and the generic kernel
splits K only from K >= 512 (K = 520: two splits of 288 and 232).

Forced stages = 3 with fewer than three K steps is not run: ``TileSrc::issue`` does not zero-fill
a stage whose k0 >= ke, it DMAs a clamped (in-range) source tile that is never read -- safe, but
not what the plan for this file required, so ``gemm_f32_fast_plan`` falls back to two stages and
``test_fast_stage_clamp`` pins that through the plan.

The cvec epilogue's beta pre-load reads ``out + 0`` for out-of-window lanes: ``out`` is the
window's first element (or the split-K workspace), 16-byte aligned by the cvec precondition, and
N >= 4, so the four floats read lie inside the window itself."""
import contextlib
import math

import pytest
import torch

import gemm_oracle as O

pytestmark = pytest.mark.gpu

# c of e_k <= 4 e_t + c u, one per quantity and product path; chosen once from the first MI355X
# run as the largest (e_k - 4 e_t) / u any case needed, rounded up to the next power of two (a
# negative need: 4 e_t alone covered every case; c = 1 is then the smallest power of two kept).
# Figures: profiles/r17/gemm_matrix.md.
C_ = {
    # split-bf16 products (fast kernel, gemm_emu8, what takes a call that leaves skinny kind 2):
    # -4.53 skinny2 misaligned C (fast kernel, 33x64x16): e_k 1.52 u, e_t 1.51 u
    "C_split": 1,
    # native f32 MFMA (fast kernel with emu off, generic kernel):
    # -6.20 generic[132x68x44 a_k b_k vec mask]: e_k 2.86 u, e_t 2.27 u
    "C_native": 1,
    # skinny kernels (fmaf chains): -5.90 skinny2[33x64x16]: e_k = e_t = 1.97 u
    "C_fma": 1,
    # 7.92 rowsum[260x196x260 A [K][M] mean 100, fast kernel, either product]: e_k 12.76 u,
    # e_t 1.21 u -- one thread adds a row's K values in k order, torch adds pairwise
    "rowsum": 8,
}
_NEED = {}


def _note(key, what, e_k, e_t):
    need = (e_k - 4 * e_t) / O.U
    if key not in _NEED or need > _NEED[key][0]:
        _NEED[key] = (need, what, e_k / O.U, e_t / O.U)


_DEFAULT = dict(mode=0, fn=0, splits=0, stages=0, bm=0, cvec=True, emu=True, waves=8)
_state = dict(_DEFAULT)


def _apply(C, s):
    C.gemm_f32_set_mode(s["mode"])
    C.gemm_f32_set_override(s["fn"], s["splits"], s["stages"])
    C.gemm_f32_set_bm(s["bm"])
    C.gemm_f32_set_cvec(s["cvec"])
    C.gemm_f32_set_emu(s["emu"])
    assert C.gemm_emu8_set_waves(s["waves"])
    _state.update(s)


@contextlib.contextmanager
def knobs(C, **kw):
    try:
        _apply(C, dict(_DEFAULT, **kw))
        yield
    finally:
        _apply(C, _DEFAULT)


def _probe_plans(C):
    out = []
    for M, N, K, a_k, b_k in [(260, 68, 260, True, True), (132, 196, 44, False, False),
                              (512, 512, 1024, True, False), (33, 64, 16, True, False)]:
        A = torch.empty((M, K) if a_k else (K, M), device="cuda")
        B = torch.empty((N, K) if b_k else (K, N), device="cuda")
        out.append(dict(C.gemm_f32_plan_for(A, B, torch.empty(M, N, device="cuda"), a_k, b_k)))
    return out


@pytest.fixture(scope="module")
def C():
    from tutorial_torch_distributed_data_parallel_amd._native import native

    c = native()
    assert c.gemm_f32_emu(), "these tests start from the default (split-bf16) products"
    before = _probe_plans(c)
    yield c
    for key, (need, what, e_k, e_t) in sorted(_NEED.items()):
        print(f"[gemm] need {key}: {need:.2f} from {what} (e_k {e_k:.2f}u, e_t {e_t:.2f}u)")
    # every knob is back at its default: the recorded state, the one getter, and the plans
    assert _state == _DEFAULT, _state
    assert c.gemm_f32_emu()
    assert _probe_plans(c) == before


def _store(t, kcontig_is_rows):
    """Logical [R, K]-like matrix t stored as is or transposed, contiguous."""
    return t.contiguous() if kcontig_is_rows else t.t().contiguous()


def _run(C, A, B, out, a_k, b_k, expect, **kw):
    plan = C.gemm_f32_plan_for(A, B, out, a_k, b_k,
                               **{k: v for k, v in kw.items()
                                  if k in ("mask", "bias", "rowsum", "gate")})
    for k, v in expect.items():
        assert plan[k] == v, f"plan[{k!r}] = {plan[k]!r}, expected {v!r}: {dict(plan)}"
    C.gemm_f32(A, B, out, a_k, b_k, **kw)
    return plan


class Case:
    """One logical problem on the GPU with its float64 / torch fp32 references, computed once."""

    def __init__(self, M, N, K, seed=0, dist="normal", a_mean=0.0, mask=False, rowsum_beta=None,
                 epilogue=True):
        P = O.Problem(M, N, K, seed=seed, dist=dist, a_mean=a_mean).to("cuda")
        self.P, self.M, self.N, self.K = P, M, N, K
        self.epilogue, self.rowsum_beta = epilogue, rowsum_beta
        kw = dict(bias=P.bias, beta=0.5, C0=P.C0, relu=True, gate=P.gate) if epilogue else {}
        if mask:
            kw["mask"] = P.mask
        if rowsum_beta is not None:
            kw.update(rowsum_beta=rowsum_beta, rowsum0=P.rowsum0)
        self.ref = O.reference(P.A, P.B, True, False, want_rowsum=rowsum_beta is not None, **kw)
        self.t32, self.t32_rs = O.torch_f32(P.A, P.B, True, False, **kw)
        self.gate_ld12 = O.strided(P.gate, ld_extra=12)  # ldgate = N + 12 != ldc = N + 8

    def operands(self, a_k, b_k):
        return _store(self.P.A, a_k), _store(self.P.B.t(), b_k)

    def frame(self, **kw):
        """The output window: pattern sentinel with C0 inside (beta = 0.5), NaN without."""
        if self.epilogue:
            f = O.framed(self.M, self.N, fill="pattern", device="cuda", **kw)
            f.view.copy_(self.P.C0)
        else:
            f = O.framed(self.M, self.N, device="cuda", **kw)
        return f

    def rowsum_frame(self):
        if self.rowsum_beta:
            f = O.framed_vec(self.M, fill="pattern", device="cuda")
            f.view.copy_(self.P.rowsum0)
        else:
            f = O.framed_vec(self.M, device="cuda")
        return f

    def call_kw(self, gate=None):
        if not self.epilogue:
            return {}
        return dict(bias=self.P.bias, beta=0.5, relu=True,
                    gate=self.gate_ld12 if gate is None else gate)

    def judge(self, f, key, what, rs=None):
        torch.cuda.synchronize()
        O.frame_intact(f)
        e_k, e_t = O.check_ref(f.view, self.ref, t32=self.t32, c=C_[key], what=what)
        _note(key, what, e_k, e_t)
        if rs is not None:
            O.frame_intact(rs)
            e_k, e_t = O.check_rowsum(rs.view, self.ref, t32=self.t32_rs, c=C_["rowsum"],
                                      what=what + " rowsum")
            _note("rowsum", what + " rowsum", e_k, e_t)


def _selection_bitwise(C, M, N, K, a_k, b_k, B_logical, expect, what, run=None):
    """A = selection matrix, no epilogue: C[m] = B[(7m + 3) mod K] bit for bit."""
    A = _store(O.selection(M, K).cuda(), a_k)
    B = _store(B_logical.t(), b_k)
    f = O.framed(M, N, device="cuda")
    if run is None:
        _run(C, A, B, f.view, a_k, b_k, expect)
    else:
        run(A, B, f.view)
    torch.cuda.synchronize()
    O.frame_intact(f)
    want = B_logical[O.selection_rows(M, K).cuda()]
    assert torch.equal(f.view, want), \
        f"{what}: {(f.view != want).sum().item()} elements differ from the selected rows of B"


def _fast_expect(N, K, fn, stages, splits, gate_after=None):
    kps = math.ceil(math.ceil(K / splits) / 32) * 32
    e = dict(skinny=0, emu8=False, fast=True, tile=fn, bm=128, bn=64 * fn,
             splits=math.ceil(K / kps), k_per_split=kps,
             stages=stages if math.ceil(kps / 32) >= 3 else 2)
    if gate_after is not None:
        e["gate_after"] = gate_after
    return e


# ---------------------------------------------------------------- a. fast-kernel plan matrix
FAST_SHAPES = [(132, 68, 44), (260, 196, 260), (132, 196, 160)]
FAST_SHAPES_BK = [(132, 66, 160), (260, 67, 260)]  # N % 4 != 0: B [N][K] only, scalar stores


@pytest.mark.parametrize("a_k,b_k", [(True, True), (True, False), (False, True), (False, False)])
def test_fast_plan_matrix(C, a_k, b_k):
    """4 layouts x FN {1, 2} x stages {2, 3} x {split-bf16, native} x cvec {on, off} x splits
    {1, 3}: full epilogue (bias, beta = 0.5, ReLU, gate with ldgate = N + 12) into a frame with
    ldc = N + 8; the wide 2^[-20, 20] operands without epilogue; the selection matrix bitwise.
    N % 4 != 0 makes ldgate % 4 != 0: those cases gate through gate_inplace (gate_after)."""
    for M, N, K in FAST_SHAPES + (FAST_SHAPES_BK if b_k else []):
        full = Case(M, N, K, seed=11)
        widec = Case(M, N, K, seed=12, dist="wide", epilogue=False)
        for emu in (True, False):
            key = "C_split" if emu else "C_native"
            for fn in (1, 2):
                for stages in (2, 3):
                    for cvec in (True, False):
                        for splits in (1, 3):
                            tag = f"fast[{M}x{N}x{K} a_k={a_k} b_k={b_k} fn={fn} st={stages} " \
                                  f"emu={emu} cvec={cvec} splits={splits}]"
                            with knobs(C, mode=2, fn=fn, splits=splits, stages=stages, cvec=cvec,
                                       emu=emu):
                                for case, name in ((full, "full"), (widec, "wide")):
                                    A, B = case.operands(a_k, b_k)
                                    f = case.frame()
                                    ex = _fast_expect(N, K, fn, stages, splits,
                                                      (N % 4 != 0) if case.epilogue else False)
                                    _run(C, A, B, f.view, a_k, b_k, ex, **case.call_kw())
                                    case.judge(f, key, f"{tag} {name}")
                                _selection_bitwise(C, M, N, K, a_k, b_k, full.P.B,
                                                   _fast_expect(N, K, fn, stages, splits), tag)


@pytest.mark.parametrize("b_k", [True, False])
def test_fast_rowsum(C, b_k):
    """Row sums exist only for A stored [K][M] and force splits == 1 (a forced split is ignored).
    A has mean 100 and spread 1: a sum in the wrong order or of the wrong tile's rows loses
    visibly against float64. The rowsum buffer is framed too."""
    for M, N, K in [(132, 68, 44), (260, 196, 260)]:
        for rb in (0.0, 0.5):
            case = Case(M, N, K, seed=13, a_mean=100.0, rowsum_beta=rb)
            A, B = case.operands(False, b_k)
            for emu in (True, False):
                for fn in (1, 2):
                    for stages in (2, 3):
                        for cvec in (True, False):
                            tag = f"rowsum[{M}x{N}x{K} b_k={b_k} rb={rb} fn={fn} st={stages} " \
                                  f"emu={emu} cvec={cvec}]"
                            with knobs(C, mode=2, fn=fn, splits=3, stages=stages, cvec=cvec,
                                       emu=emu):
                                f, rs = case.frame(), case.rowsum_frame()
                                ex = _fast_expect(N, K, fn, stages, 1, False)
                                _run(C, A, B, f.view, False, b_k, ex, rowsum=rs.view,
                                     rowsum_beta=rb, **case.call_kw())
                                case.judge(f, "C_split" if emu else "C_native", tag, rs)


def test_fast_stage_clamp(C):
    """A forced third stage with fewer than three K steps per split falls back to two."""
    for K, splits, want in [(32, 1, 2), (44, 1, 2), (64, 1, 2), (96, 1, 3), (260, 1, 3),
                            (260, 3, 3), (160, 3, 2)]:
        A = torch.empty(132, K, device="cuda")
        B = torch.empty(68, K, device="cuda")
        out = torch.empty(132, 68, device="cuda")
        with knobs(C, mode=2, fn=1, splits=splits, stages=3):
            plan = C.gemm_f32_plan_for(A, B, out, True, True)
        assert plan["fast"] and plan["stages"] == want, (K, splits, dict(plan))


# ---------------------------------------------------------------- b. the 256-row kernel
def test_fast_bm256(C):
    """gemm_f32_set_bm(256): the FM = 4 kernel (K-contiguous A, FN = 1, no split, no rowsum)."""
    M = 260
    for N, K in [(68, 44), (68, 260), (66, 44), (66, 260)]:
        case = Case(M, N, K, seed=21)
        for b_k in ((True, False) if N % 4 == 0 else (True,)):
            A, B = case.operands(True, b_k)
            for emu in (True, False):
                for cvec in (True, False):
                    tag = f"bm256[{M}x{N}x{K} b_k={b_k} emu={emu} cvec={cvec}]"
                    with knobs(C, mode=2, bm=256, cvec=cvec, emu=emu):
                        f = case.frame()
                        ex = dict(fast=True, bm=256, bn=64, tile=1, splits=1, skinny=0,
                                  emu8=False, gate_after=N % 4 != 0)
                        _run(C, A, B, f.view, True, b_k, ex, **case.call_kw())
                        case.judge(f, "C_split" if emu else "C_native", tag)
                        _selection_bitwise(C, M, N, K, True, b_k, case.P.B,
                                           dict(fast=True, bm=256), tag)
    # what gemm_f32_fast_plan says falls back to 128 rows
    case = Case(M, 68, 260, seed=22, rowsum_beta=0.0)
    with knobs(C, mode=2, bm=256):
        A, B = case.operands(False, True)
        f, rs = case.frame(), case.rowsum_frame()
        _run(C, A, B, f.view, False, True, dict(fast=True, bm=128), **case.call_kw())
        case.judge(f, "C_split", "bm256 fallback: A [K][M]")
        f = case.frame()
        _run(C, A, B, f.view, False, True, dict(fast=True, bm=128, splits=1), rowsum=rs.view,
             **case.call_kw())
        case.judge(f, "C_split", "bm256 fallback: rowsum", rs)
    with knobs(C, mode=2, bm=256, splits=3):
        A, B = case.operands(True, True)
        f = case.frame()
        _run(C, A, B, f.view, True, True, dict(fast=True, bm=128, splits=3), **case.call_kw())
        case.judge(f, "C_split", "bm256 fallback: forced split")


# ---------------------------------------------------------------- c. gate on every route
def test_gate_on_every_implementation(C):
    """One problem (132 x 68 x 160, N = 66 where a scalar path needs it) through each of the six
    gate implementations, the plan asserted each time; the gate holds 0.0, -0.0, NaN, a negative
    and a positive subnormal inside the last ragged tile, under positive pre-activations."""
    case = Case(132, 68, 160, seed=31)
    case66 = Case(132, 66, 160, seed=31)
    gate66 = O.strided(case66.P.gate, ld_extra=14)  # ldgate = 80: 16-B rows, stays in the kernel
    outs = {}

    def route(name, cs, a_k, b_k, expect, key="C_split", gate=None, **kn):
        with knobs(C, **kn):
            A, B = cs.operands(a_k, b_k)
            f = cs.frame()
            _run(C, A, B, f.view, a_k, b_k, expect, **cs.call_kw(gate))
            cs.judge(f, key, f"gate[{name}]")
            outs[name] = f.view.clone()

    fast1 = dict(fast=True, skinny=0, tile=1, splits=1, gate_after=False)
    route("fast cvec", case, True, True, fast1, mode=2, fn=1, splits=1)
    route("fast scalar", case, True, True, fast1, mode=2, fn=1, splits=1, cvec=False)
    route("fast scalar N=66", case66, True, True, fast1, gate=gate66, mode=2, fn=1, splits=1)
    route("fast paired", case, True, False, dict(fast1, tile=2), mode=2, fn=2, splits=1,
          cvec=False)
    sk = dict(fast=True, splits=3, k_per_split=64, gate_after=False)
    route("splitk vector", case, True, True, sk, mode=2, fn=1, splits=3)
    route("splitk scalar", case66, True, True, sk, gate=gate66, mode=2, fn=1, splits=3)
    route("generic", case, True, True, dict(fast=False, skinny=0, tile=1, splits=1,
                                            gate_after=False), key="C_native", mode=1)
    after = dict(fast1, gate_after=True)
    route("gate_after ld", case, True, True, after, gate=O.strided(case.P.gate, ld_extra=1),
          mode=2, fn=1, splits=1)
    route("gate_after ptr", case, True, True, after,
          gate=O.strided(case.P.gate, ld_extra=12, offset=1), mode=2, fn=1, splits=1)
    # the same fn = 1 kernel, products and k order: whichever way the tile is stored and gated,
    # the same elements are zero
    for other in ("fast scalar", "gate_after ld", "gate_after ptr"):
        assert torch.equal(outs["fast cvec"] == 0, outs[other] == 0), other
    for a, b in (("fast cvec", "splitk vector"), ("fast cvec", "fast paired"),
                 ("fast cvec", "generic"), ("fast scalar N=66", "splitk scalar")):
        za, zb = outs[a] == 0, outs[b] == 0
        closed = O.closed(case.P.gate if outs[a].shape[1] == 68 else case66.P.gate)
        assert torch.equal(za & closed, zb & closed) and bool((za & closed).eq(closed).all())
    for (M, N, K), (a_k, b_k), kind in [((132, 10, 160), (True, True), 1),
                                        ((132, 68, 12), (True, False), 2),
                                        ((12, 68, 160), (False, False), 3)]:
        route(f"skinny {kind}", Case(M, N, K, seed=32), a_k, b_k,
              dict(skinny=kind, gate_after=False), key="C_fma")


# ---------------------------------------------------------------- d. generic kernel
@pytest.mark.parametrize("M,N,K,tile,splits", [(37, 68, 44, 2, 1), (132, 68, 44, 1, 1),
                                               (512, 512, 44, 0, 1), (37, 68, 520, 2, 2)])
def test_generic_kernel(C, M, N, K, tile, splits):
    """mode = 1: the three tile configurations (the tile depends on M and N alone; 128 x 128
    needs 512 x 512), VEC and non-VEC loads (A misaligned by one float, then lda = K + 1), the
    mask with ldmask = K + 4, rowsum of the masked A, split-K (K >= 512) on and off."""
    big = M >= 512
    for mask in ((True,) if big else (False, True)):
        case = Case(M, N, K, seed=41, mask=mask, rowsum_beta=0.5 if splits == 1 else None)
        for a_k, b_k in [(True, True), (True, False), (False, True), (False, False)]:
            A0, B = case.operands(a_k, b_k)
            m0 = _store(case.P.mask, a_k)
            for how in (("vec",) if big and not (a_k and b_k) else ("vec", "ptr", "ld")):
                A = {"vec": A0, "ptr": O.strided(A0, 0, offset=1), "ld": O.strided(A0, 1)}[how]
                if how != "vec":  # the launch takes VEC only with 16-B rows of A, B and the mask
                    assert A.data_ptr() % 16 != 0 or A.stride(0) % 4 != 0
                kw = case.call_kw()
                if mask:
                    kw["mask"] = O.strided(m0, ld_extra=4)
                f = case.frame()
                rs = case.rowsum_frame() if splits == 1 else None
                if rs is not None:
                    kw.update(rowsum=rs.view, rowsum_beta=0.5)
                ex = dict(fast=False, skinny=0, emu8=False, tile=tile, splits=splits,
                          gate_after=False)
                if splits > 1:
                    ex["k_per_split"] = 288
                with knobs(C, mode=1):
                    _run(C, A, B, f.view, a_k, b_k, ex, **kw)
                case.judge(f, "C_native",
                           f"generic[{M}x{N}x{K} a_k={a_k} b_k={b_k} {how} mask={mask}]", rs)
        if not big:
            with knobs(C, mode=1):
                for a_k, b_k in [(True, True), (False, False)]:
                    _selection_bitwise(C, M, N, K, a_k, b_k, case.P.B,
                                       dict(fast=False, tile=tile, splits=splits),
                                       f"generic[{M}x{N}x{K} a_k={a_k} b_k={b_k}]")


# ---------------------------------------------------------------- e. skinny kernels
SKINNY = {1: ((77, 13, 260), (True, True)), 2: ((33, 64, 16), (True, False)),
          3: ((16, 100, 300), (False, False))}


def _key_of(plan):
    return "C_fma" if plan["skinny"] else "C_split" if plan["fast"] else "C_native"


@pytest.mark.parametrize("kind", [1, 2, 3])
def test_skinny_kernels(C, kind):
    """Full epilogue and frames on the three kinds; each kind's boundary (16 in, 17 out); the
    alignment conditions of gemm_skinny_kind (a misaligned C or bias leaves kind 2). Whatever
    kernel takes the call instead is checked by the same rule."""
    (M, N, K), (a_k, b_k) = SKINNY[kind]
    edge = {1: [(M, 16, K), (M, 17, K)], 2: [(M, N, 16), (M, N, 17)],
            3: [(16, N, K), (17, N, K)]}[kind]
    for i, (m, n, k) in enumerate([(M, N, K)] + edge):
        inside = i < 2
        case = Case(m, n, k, seed=51, rowsum_beta=0.5 if kind == 3 else None)
        A, B = case.operands(a_k, b_k)
        f = case.frame()
        kw = case.call_kw()
        rs = None
        if kind == 3:
            rs = case.rowsum_frame()
            kw.update(rowsum=rs.view, rowsum_beta=0.5)
        with knobs(C):
            plan = _run(C, A, B, f.view, a_k, b_k,
                        dict(skinny=kind, gate_after=False) if inside else {}, **kw)
        assert (plan["skinny"] == kind) == inside, (m, n, k, dict(plan))
        case.judge(f, _key_of(plan), f"skinny{kind}[{m}x{n}x{k}]", rs)
        if inside:
            _selection_bitwise(C, m, n, k, a_k, b_k, case.P.B, dict(skinny=kind),
                               f"skinny{kind}[{m}x{n}x{k}]")
    if kind == 2:
        case = Case(M, N, K, seed=52)
        A, B = case.operands(a_k, b_k)
        with knobs(C):
            f = case.frame(pad_cols=1)  # C misaligned by one float
            plan = _run(C, A, B, f.view, a_k, b_k, {}, **case.call_kw())
            assert plan["skinny"] != 2, dict(plan)
            case.judge(f, _key_of(plan), "skinny2 misaligned C")
            kw = case.call_kw()
            bias = torch.zeros(N + 4, device="cuda")[1:N + 1]
            bias.copy_(case.P.bias)
            kw["bias"] = bias
            f = case.frame()
            plan = _run(C, A, B, f.view, a_k, b_k, {}, **kw)
            assert plan["skinny"] != 2, dict(plan)
            case.judge(f, _key_of(plan), "skinny2 misaligned bias")


# ---------------------------------------------------------------- f. gemm_emu8 directly
K8 = 32  # kBK8, the K step of csrc/gemm_emu8.hip (emu8.h: K % 32 == 0)


@pytest.mark.parametrize("b_k,N", [(True, 262), (False, 260)])
def test_gemm_emu8_small_ragged(C, b_k, N):
    """The 256 x 256 kernel at M = 260 (two row tiles, 4 ragged rows), two column tiles, K = two
    and three K steps, beta 0 / 1, 4 and 8 waves, into a framed strided C: against float64, bit
    for bit on the selection input, and bitwise equal to the 128 x 128 fast kernel."""
    M = 260
    for K in (2 * K8, 3 * K8):
        P = O.Problem(M, N, K, seed=61).to("cuda")
        A, B = P.A.contiguous(), _store(P.B.t(), b_k)
        for beta in (0.0, 1.0):
            kw = dict(beta=beta, C0=P.C0) if beta else {}
            ref = O.reference(P.A, P.B, True, False, **kw)
            t32, _ = O.torch_f32(P.A, P.B, True, False, **kw)

            def frame():
                f = O.framed(M, N, fill="pattern" if beta else float("nan"), device="cuda")
                if beta:
                    f.view.copy_(P.C0)
                return f

            fast = frame()
            with knobs(C, mode=2, fn=2, splits=1):
                _run(C, A, B, fast.view, True, b_k, dict(fast=True, emu8=False, tile=2, bm=128),
                     beta=beta)
            for waves in (4, 8):
                what = f"emu8[{M}x{N}x{K} b_k={b_k} beta={beta} waves={waves}]"
                f = frame()
                with knobs(C, waves=waves):
                    C.gemm_emu8(A, B, f.view, b_k, beta)
                torch.cuda.synchronize()
                O.frame_intact(f)
                e_k, e_t = O.check_ref(f.view, ref, t32=t32, c=C_["C_split"], what=what)
                _note("C_split", what, e_k, e_t)
                assert torch.equal(f.view, fast.view), what + ": differs from the fast kernel"
        for waves in (4, 8):
            with knobs(C, waves=waves):
                _selection_bitwise(C, M, N, K, True, b_k, P.B, None,
                                   f"emu8[{M}x{N}x{K} b_k={b_k} waves={waves}]",
                                   run=lambda a, b, out: C.gemm_emu8(a, b, out, b_k, 0.0))
