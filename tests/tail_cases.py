"""fp64 oracles, bounds and case generators for the trunk tail's kernels: network.5 + critic
forward (fc.hip mbk_fc_fwd), the NT GEMM with its epilogues (gemm.hip), the split-K weight
gradients (fc.hip), the critic backward, the column sums and the index gather (gridnet.hip).

The oracles are written from the definitions, in plain torch float64, on the kernels' own
operands; each returns A, the same expression on absolute values, which the bounds scale.
tests/test_tail_cases.py checks them on the CPU against nn.Linear + autograd on the reference's
NCHW flatten; tests/test_gpu_tail.py holds every launcher to them.

Two kinds of case (conv_cases.Case):

* exact: activations and gradients are integers in [-2, 2], weights in {0, +-0.5, +-1} at half
  density, biases multiples of 0.5. Every fp32 partial sum is exact in any order
  (``assert_fp32_exact``), so a kernel must equal the oracle rounded once to its output type, bit
  for bit. About a fifth of the activations (the relu inputs and masks) are exactly zero, every
  second one written as -0.0 (0x8000): neither zero is "> 0". network.5's bias carries an offset
  of 0, 64, .. 320 per hidden unit, so pre-activations lie up to 320 + 40: halves above 128 and
  odd integers above 256 are not bf16 numbers, f is rounded for real and the x.5 / odd values are
  round-to-nearest-even ties, and the critic on the rounded f differs from the one on the
  unrounded f. No operand is a bf16 subnormal.
* round: random-normal operands rounded to bf16 (weights x 0.2, biases x 0.1), a tenth of the
  relu inputs and masks zeroed (half of them -0.0), against the bounds below.

Bounds (conv_cases.bf16_bound / f32_bound: one round-to-nearest bf16 store 2^-8 |ref|, 2^-23 A
per summed term, twice fp32's first-order bound in any order):

* f: bf16_bound(ref, A, I + 1) (I products and the bias; relu is 1-Lipschitz).
* v: f32_bound(sum |f||wc| + |bc|, O + 1), on the kernel's own stored bf16 f.
* GEMM: n = K + 1, + 1 with a bias, + 1 with the accumulated c0 (each is one more fp32 add of a
  term that A carries); bf16_bound(ref, A, n) or f32_bound(A, n); A is zero at masked entries,
  so those must be exactly zero.
* dW: f32_bound(sum_n |g||x|, N), db: f32_bound(sum_n |g|, N); one more term and |out0| in A
  when the result is accumulated into out0.
* dh: bf16_bound(ref, |dv w2| + |gadd|, 2) where h > 0, exactly 0 elsewhere; dW2, db2 and column
  sums: f32_bound over R terms.
* map_gather: a copy, bit for bit (a bf16 destination: .bfloat16() of the fp32 source).
"""
import torch

from conv_cases import (U_BF16, U_SUM, Case, assert_bf16_exact, assert_fp32_exact,  # noqa: F401
                        bf16_bound, f32_bound, round_trunc_bf16, worst_ratio)

BF = torch.bfloat16


# ------------------------------------------------------------------ oracles
def fc_fwd_ref(x, w5, b5, relu_in):
    """f = relu(relu?(x) . W5^T + b5) [F, O] and A (pre-relu magnitudes)."""
    x = x.double()
    if relu_in:
        x = x.clamp_min(0)
    wq, b = w5.bfloat16().double(), b5.double()
    return (x @ wq.t() + b).clamp_min(0), x.abs() @ wq.abs().t() + b.abs()


def critic_ref(f, wc, bc):
    """v = f . wc + bc [F] on the stored (bf16) activations f, and A."""
    f, wc, bc = f.double(), wc.double().reshape(-1), bc.double().reshape(())
    return f @ wc + bc, f.abs() @ wc.abs() + bc.abs()


def gemm_nt_ref(a, b, bias=None, relu=False, mask=None, c0=None):
    """A . B^T (+ bias) (relu) (. [mask > 0]) (+ c0) [M, N] and its A."""
    a, b = a.double(), b.double()
    y, A = a @ b.t(), a.abs() @ b.abs().t()
    if bias is not None:
        y, A = y + bias.double(), A + bias.double().abs()
    if relu:
        y = y.clamp_min(0)
    if mask is not None:
        m = (mask.double() > 0).double()
        y, A = y * m, A * m
    if c0 is not None:
        y, A = y + c0.double(), A + c0.double().abs()
    return y, A


def wgrad_ref(g, x, relu_x):
    """dW = g^T relu?(x) [O, I], db = g^T 1 [O] and their A: (dW, db, A_w, A_b)."""
    g, x = g.double(), x.double()
    if relu_x:
        x = x.clamp_min(0)
    return g.t() @ x, g.sum(0), g.abs().t() @ x.abs(), g.abs().sum(0)


def value_bwd_ref(dv, h, w2, gadd=None, gadd_rows=0):
    """Critic output layer backward: dh = (dv w2 + gadd[rows < gadd_rows]) [h > 0], dW2 = dv^T h,
    db2 = sum dv: (dh, A_h, dW2, A_w, db2, A_b)."""
    dv, h, w2 = dv.double().reshape(-1), h.double(), w2.double().reshape(-1)
    d = dv[:, None] * w2[None, :]
    A = d.abs()
    if gadd is not None and gadd_rows > 0:
        d, A = d.clone(), A.clone()
        d[:gadd_rows] += gadd[:gadd_rows].double()
        A[:gadd_rows] += gadd[:gadd_rows].double().abs()
    m = (h > 0).double()
    return d * m, A * m, dv @ h, dv.abs() @ h.abs(), dv.sum(), dv.abs().sum()


def colsum_ref(x, C):
    """Column sums of the first C columns of x [R, ld] and A."""
    x = x.double()[:, :C]
    return x.sum(0), x.abs().sum(0)


def map_gather_ref(src, m):
    """dst[i] = src.flat[m[i]], 0 where m[i] = -1 (same dtype as src)."""
    flat, m = src.reshape(-1), m.reshape(-1).long()
    return torch.where(m >= 0, flat[m.clamp_min(0)], torch.zeros((), dtype=src.dtype))


def gemm_terms(K, bias=False, acc=False):
    return K + 1 + int(bias) + int(acc)


# ------------------------------------------------------------------ operands
class TailCase(Case):
    """conv_cases.Case plus the tail's operand forms."""

    def zeros_in(self, t, share):
        """Zero a share of t's elements (share = 0: keep what is zero already) and write every
        second zero, by a coin, as -0.0."""
        if share > 0:
            t = torch.where(torch.rand(t.shape, generator=self.g) < share, torch.zeros_like(t), t)
        neg = (t == 0) & (torch.rand(t.shape, generator=self.g) < 0.5)
        return torch.where(neg, torch.full_like(t, -0.0), t)

    def gated(self, shape):
        """bf16 relu inputs / masks: about a fifth (exact) or a tenth (round) exactly zero, half
        of those -0.0."""
        return self.zeros_in(self.acts(shape), 0.0 if self.exact else 0.1)

    def mat(self, o, i):
        """fp32 weights [o, i] that are bf16 numbers."""
        if self.exact:
            v = torch.tensor([-1.0, -0.5, 0.5, 1.0])[torch.randint(0, 4, (o, i), generator=self.g)]
            return (v * (torch.rand((o, i), generator=self.g) < 0.5)).float()
        return (torch.randn((o, i), generator=self.g) * 0.2).bfloat16().float()

    def vec(self, n):
        """fp32 biases [n]."""
        if self.exact:
            return (self.ints((n,), -4, 4) / 2).float()
        return (torch.randn(n, generator=self.g) * 0.1).bfloat16().float()

    def fc_bias(self, n):
        """network.5's bias: the exact case adds 0, 64, .. 320 per hidden unit (module docstring)."""
        b = self.vec(n)
        return b + 64.0 * self.ints((n,), 0, 5).float() if self.exact else b

    def f32(self, shape):
        """fp32 gradients / prefilled outputs (bf16 numbers held in fp32)."""
        return self.acts(shape).float()


def assert_no_subnormal(*ts):
    for t in ts:
        a = t.double().abs()
        assert not bool(((a > 0) & (a < 2.0 ** -126)).any())


def signed_zero_counts(t):
    """(+0 count, -0 count) of a bf16 tensor."""
    bits = t.contiguous().view(torch.int16)
    return int((bits == 0).sum()), int((bits == -32768).sum())


# --- mbk_fc_fwd
FC_RB = [(256, 32), (256, 64), (256, 96), (256, 128), (128, 32), (128, 128)]   # fc_fwd_rb_kernel
FC_GENERIC = [(256, 160), (256, 288), (128, 160), (512, 64)]                  # fc_fwd_kernel
FC_F = [1, 15, 16, 17, 31, 32, 33, 47]
FC_LONG = [(256, 128), (256, 288)]  # one per kernel family at F = 2 CUs 32 + 49


def fc_operands(kind, O, I, F=max(FC_F)):
    """(x [F, I] bf16, w5 [O, I], b5 [O], wc [O], bc [1]) of one mbk_fc_fwd case."""
    c = TailCase(kind, 7000 + 3 * O + I + (0 if F == max(FC_F) else 1))
    x, w5, b5, wc, bc = c.gated((F, I)), c.mat(O, I), c.fc_bias(O), c.mat(1, O)[0], c.vec(1)
    assert_no_subnormal(x, w5, b5, wc, bc)
    return x, w5, b5, wc, bc


# --- mbk_gemm_nt / mbk_gemm_nt_mask: (M, N, K, out, bias, relu, mask, ldc - N, mask offset)
# out: 'bf16', 'f32' or 'acc' (fp32 accumulated into c0); mask offset in elements (1: the mask
# pointer is 2 bytes off a 16-byte boundary, which sends a bf16 output to the per-element epilogue)
GEMM_CASES = [
    # 256 x 32 tile (N <= 32)
    (1, 8, 8, "bf16", 1, 0, 0, 0, 0),        # vectorised
    (257, 32, 40, "bf16", 0, 0, 1, 8, 0),    # vectorised, mask, row gaps
    (255, 31, 24, "bf16", 1, 1, 1, 0, 0),    # per element: N % 8
    (129, 8, 32, "bf16", 0, 1, 1, 3, 0),     # per element: ldc = N + 3
    (256, 32, 64, "bf16", 1, 0, 1, 0, 1),    # per element: mask pointer offset
    (513, 1, 64, "f32", 1, 0, 0, 0, 0),
    (127, 32, 256, "f32", 0, 1, 1, 8, 0),
    (256, 31, 288, "acc", 1, 1, 0, 0, 0),
    # 256 x 64 tile (N <= 64)
    (256, 64, 256, "bf16", 1, 1, 1, 0, 0),   # vectorised
    (513, 64, 8, "bf16", 0, 0, 0, 8, 0),     # vectorised, row gaps, no epilogue option
    (257, 33, 40, "bf16", 0, 0, 1, 0, 0),    # per element: N % 8
    (128, 64, 32, "bf16", 1, 0, 0, 3, 0),    # per element: ldc = N + 3
    (127, 64, 24, "bf16", 0, 1, 1, 0, 1),    # per element: mask pointer offset
    (513, 64, 32, "f32", 0, 0, 1, 8, 0),
    (128, 33, 64, "acc", 1, 1, 0, 0, 0),
    # 128 x 128 tile
    (129, 72, 8, "bf16", 0, 0, 1, 8, 0),     # vectorised, mask, row gaps
    (513, 264, 288, "bf16", 1, 1, 1, 0, 0),  # vectorised, three column tiles, five row tiles
    (255, 65, 256, "bf16", 1, 0, 0, 0, 0),   # per element: N % 8
    (128, 128, 32, "bf16", 0, 0, 1, 3, 0),   # per element: ldc = N + 3
    (256, 136, 24, "bf16", 0, 1, 1, 0, 1),   # per element: mask pointer offset
    (1, 129, 64, "f32", 1, 1, 1, 0, 0),
    (257, 136, 40, "acc", 0, 0, 0, 8, 0),
]


def gemm_operands(kind, idx):
    """(a [M, K] bf16, b [N, K] bf16, bias [N] | None, mask [M, N] bf16 | None, c0 [M, N] fp32 |
    None) of GEMM_CASES[idx]."""
    M, N, K, out, bias, relu, mask, _, _ = GEMM_CASES[idx]
    c = TailCase(kind, 8000 + idx)
    a, b = c.acts((M, K)), c.mat(N, K).bfloat16()
    bv = c.vec(N) if bias else None
    mk = c.gated((M, N)) if mask else None
    c0 = (c.f32((M, N)) / 2) if out == "acc" else None
    assert_no_subnormal(a, b)
    return a, b, bv, mk, c0


# --- mbk_fc_wgrad / mbk_fc_wgrad_ex / mbk_fc_wgrad_wide
WGRAD_OI = [(256, 128), (1, 256), (77, 40), (65, 72), (256, 288)]
WGRAD_N = [1, 31, 32, 33, 127, 128, 129, 300]
WIDE_I = [32, 64, 128]
WIDE_N = [1, 100, 127, 128, 129, 513, 1300]
STAGE = 128  # rows per LDS stage of both weight-gradient kernels


def stages(n):
    return (n + STAGE - 1) // STAGE


def wgrad_nparts(n):
    """Hand-passed part counts: one, the stage count, more parts than stages (empty parts), the
    two-level reduce with a partial last split (65 = 2 x 32 + 1, 97 = 3 x 32 + 1), and two parts
    where a part boundary lies inside the rows (N = 129: 128 | 1; N = 300: 256 | 44)."""
    ps = [1, stages(n), stages(n) + 2, 65, 97]
    if n in (129, 300):
        ps.append(2)
    return sorted(set(ps))


def wide_nparts(n):
    return sorted({1, stages(n), stages(n) + 3, 65, 97})


# At the row counts above every part past the third is empty, so the two-level reduce's partial
# last split (parts 64 / 96) holds zeros only and a reduce that dropped it would pass. Here part
# p is stage p and the last part, alone in the last split, holds the last 5 rows: {nparts: N}.
LONG_PARTS = {65: 64 * STAGE + 5, 97: 96 * STAGE + 5}


def wgrad_operands(kind, O, I, N):
    """(g [N, O] bf16, x [N, I] bf16 with signed zeros, out0 [O, I] fp32 for accumulate)."""
    c = TailCase(kind, 9000 + 5 * O + I)
    nmax = max(WGRAD_N + WIDE_N + [N])
    g, x, out0 = c.acts((nmax, O)), c.gated((nmax, I)), c.f32((O, I)) / 2
    return g[:N], x[:N], out0


# --- mbk_value_bwd
VALUE_K = [8, 96, 256, 2048]
VALUE_R = [1, 7, 1023, 1024, 1025, 2049]


def value_operands(kind, K, R):
    """(dv [R] fp32, h [R, K] bf16 with signed zeros, w2 [K] fp32, gadd [R, K] fp32): gadd holds
    R rows whatever gadd_rows is, so rows past gadd_rows are there to be wrongly added."""
    c = TailCase(kind, 10000 + K)
    rmax = max(VALUE_R)
    dv, h, w2 = c.f32((rmax,)), c.gated((rmax, K)), c.mat(1, K)[0]
    gadd = c.f32((rmax, K))
    return dv[:R], h[:R], w2, gadd[:R]


def value_gadd_rows(R):
    return sorted({1, max(1, R - 5), R})


# --- mbk_colsum: (name, C, ld, fp32 input, base offset in elements)
COLSUM_CASES = [
    ("vec256", 256, 256, 0, 0), ("vec78_80", 78, 80, 0, 0), ("vec78_96", 78, 96, 0, 0),
    ("scalar257", 257, 264, 0, 0), ("scalar_ld83", 78, 83, 0, 0), ("scalar_off1", 72, 80, 0, 1),
    ("f32_78", 78, 80, 1, 0), ("f32_257", 257, 257, 1, 0),
]
COLSUM_R = [0, 1, 1023, 1024, 1025, 5000]


def colsum_operands(kind, name):
    """x [max R, ld] (bf16 or fp32), every column filled (the columns past C too)."""
    _, C, ld, f32, _ = next(t for t in COLSUM_CASES if t[0] == name)
    c = TailCase(kind, 11000 + C + ld + f32)
    x = c.acts((max(COLSUM_R), ld))
    return x.float() if f32 else x


# --- the maps
MAP_SHAPES = [(32, 1, 1), (32, 2, 2), (32, 1, 2), (32, 2, 1), (32, 3, 3)]  # (c, ho, wo)
CHAIN_SHAPES = [(1, 2), (2, 2), (3, 3)]  # I = 64, 128 (wide weight gradient), 288 (fallback)
CHAIN_N = 1300


def chain_operands(kind, ho, wo, n=CHAIN_N, O=256, c=32):
    """(y [n, ho, wo, c] bf16 NHWC, w5 [O, c ho wo] in the parameter's NCHW-flatten layout, b5,
    wc, bc, dh [n, O] bf16)."""
    t = TailCase(kind, 12000 + 10 * ho + wo)
    y, w5 = t.gated((n, ho, wo, c)), t.mat(O, c * ho * wo)
    return y, w5, t.fc_bias(O), t.mat(1, O)[0], t.vec(1), t.acts((n, O))


def chain_ref(y, w5, b5, dh):
    """fp64 autograd of the reference-layout nn.Linear on the NCHW flatten with the bf16-rounded
    weights: (f, dy in NHWC, dW5 in parameter layout, db5). dh is the gradient at the Linear's
    output (the relu behind it is the caller's)."""
    n, ho, wo, c = y.shape
    x = y.double().permute(0, 3, 1, 2).reshape(n, -1).clone().requires_grad_(True)
    w = w5.bfloat16().double().clone().requires_grad_(True)
    b = b5.double().clone().requires_grad_(True)
    pre = torch.nn.functional.linear(torch.relu(x), w, b)
    pre.backward(dh.double())
    # relu'(0) = 0 in ATen too: a zero input of either sign passes no gradient
    dy = x.grad.view(n, c, ho, wo).permute(0, 2, 3, 1).reshape(n, -1)
    return torch.relu(pre).detach(), dy, w.grad, b.grad
