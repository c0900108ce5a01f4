"""fp64 oracles and case generators for the conv trunk's per-layer kernels (conv.hip).

The oracles are written from the definitions, in plain torch float64, on the kernels' NHWC
operands; tests/test_conv_cases.py checks them against F.conv2d / max_pool2d and autograd on the
CPU, tests/test_gpu_conv_layers.py holds every per-layer launcher to them.

Two kinds of case:

* exact: every operand is a small multiple of 0.5 (activations and gradients integers in
  [-2, 2], weights in {0, +-0.5, +-1} at half density, bias a multiple of 0.5 in [-2, 2]). Every
  fp32 partial sum is then exact in any order (``assert_fp32_exact``), so a kernel must equal
  the oracle, rounded once to its output type, bit for bit. Values repeat heavily, so pool
  windows tie all the time and the argmax bytes test the tie rule.
* round: random-normal operands rounded to bf16, against derived bounds (``bf16_bound``,
  ``f32_bound``).
"""
import torch
import torch.nn.functional as F

from microbeast_amd.ops.encoder import EMPTY_WORD, PLANE_GROUPS
from microbeast_amd.ops.obs import bits_to_planes

U_BF16 = 2.0 ** -8   # unit roundoff of one round-to-nearest bf16 store (8 significand bits)
U_SUM = 2.0 ** -23   # per summed term: twice fp32's first-order 2^-24 (MFMA-internal margin)

TAPS = tuple((ky - 1, kx - 1) for ky in range(3) for kx in range(3))  # scan order, ky outer


# ------------------------------------------------------------------ layer matrix
# name -> (H, W, channels): the maps the trunk supports (three stages at 8, 10, 16 and 24, 24 with
# four stages) and GridNet's first layer (32 output channels on a padded 16x16 map)
ENCODERS = {
    "s8": (8, 8, (16, 32, 32)),
    "s10": (10, 10, (16, 32, 32)),
    "s16": (16, 16, (16, 32, 32)),
    "s24": (24, 24, (16, 32, 32)),
    "s24x4": (24, 24, (16, 32, 32, 32)),
    "grid16": (16, 16, (32,)),
    # an odd map in the 17..32-wide row kernel's range (its pooled map is 9 wide, not 8)
    "w17": (17, 17, (16,)),
}
NONSQUARE = {
    "8x16": (8, 16, (16, 32, 32)),
    "16x8": (16, 8, (16, 32, 32)),
    "10x16": (10, 16, (16, 32, 32)),
}


def trunk_layers(h, w, channels):
    """(index, cin, cout, H, W, bits, relu_in, pool) of every conv of a trunk, in HipEncoder's
    layer order: per stage the pooled stage conv, then four residual convs on the pooled map."""
    out, H, W, cin, bits = [], h, w, 32, True
    for co in channels:
        out.append((len(out), cin, co, H, W, bits, False, True))
        H, W = (H + 1) // 2, (W + 1) // 2
        for _ in range(4):
            out.append((len(out), co, co, H, W, False, True, False))
        cin, bits = co, False
    return out


def distinct_layers(encoders):
    """[(encoder name, layer index)] with one entry per distinct (cin, cout, H, W, bits, pool)."""
    seen, out = set(), []
    for name, (h, w, ch) in encoders.items():
        for i, *key in trunk_layers(h, w, ch):
            key = tuple(key)
            if key not in seen:
                seen.add(key)
                out.append((name, i))
    return out


# ------------------------------------------------------------------ oracles
def _shift(x, dy, dx):
    """x[n, y + dy, x + dx, c], zero outside the map (|dy|, |dx| <= 1)."""
    n, H, W, _ = x.shape
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    return xp[:, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W]


def planes_nhwc(obs, H, W, planes=27):
    """Observation words [N, H*W] -> their bit planes [N, H, W, planes] in float64."""
    return bits_to_planes(obs.cpu(), H, W, torch.float64, planes).permute(0, 2, 3, 1).contiguous()


def conv_fwd_ref(x, w, bias=None, relu_in=False, add=None, taps=TAPS):
    """y[n, y, x, co] = sum_t sum_ci relu?(x)[n, y + dy_t, x + dx_t, ci] w[co, ci, t] + bias + add
    with the bf16-rounded weights; also A, the same expression on absolute values."""
    x = x.double()
    if relu_in:
        x = x.clamp_min(0)
    wq = w.bfloat16().double()
    n, H, W, _ = x.shape
    y = torch.zeros(n, H, W, w.shape[0], dtype=torch.float64)
    A = torch.zeros_like(y)
    for t, (dy, dx) in enumerate(taps):
        xs, wt = _shift(x, dy, dx), wq[:, :, t // 3, t % 3].t()
        y += xs @ wt
        A += xs.abs() @ wt.abs()
    if bias is not None:
        y += bias.double()
        A += bias.double().abs()
    if add is not None:
        y += add.double()
        A += add.double().abs()
    return y, A


def conv_dgrad_ref(dy, w, mask_src=None, add=None):
    """dx[n, y, x, ci] = sum_t sum_co dy[n, y - dy_t, x - dx_t, co] w[co, ci, t], times
    (mask_src > 0), plus add; and its A."""
    dy = dy.double()
    wq = w.bfloat16().double()
    n, H, W, _ = dy.shape
    dx = torch.zeros(n, H, W, w.shape[1], dtype=torch.float64)
    A = torch.zeros_like(dx)
    for t, (oy, ox) in enumerate(TAPS):
        ds, wt = _shift(dy, -oy, -ox), wq[:, :, t // 3, t % 3]
        dx += ds @ wt
        A += ds.abs() @ wt.abs()
    if mask_src is not None:
        m = (mask_src.double() > 0).double()
        dx, A = dx * m, A * m
    if add is not None:
        dx += add.double()
        A += add.double().abs()
    return dx, A


def conv_wgrad_ref(x, dy, relu_in=False):
    """dW[co][ci][ky][kx] = sum_p dy[p][co] relu?(x)[p + t][ci], db[co] = sum_p dy[p][co], and
    their A: (dW, db, A_w, A_b)."""
    x, dy = x.double(), dy.double()
    if relu_in:
        x = x.clamp_min(0)
    cin, cout = x.shape[-1], dy.shape[-1]
    dW = torch.zeros(cout, cin, 3, 3, dtype=torch.float64)
    A = torch.zeros_like(dW)
    df = dy.reshape(-1, cout)
    for t, (oy, ox) in enumerate(TAPS):
        xs = _shift(x, oy, ox).reshape(-1, cin)
        dW[:, :, t // 3, t % 3] = df.t() @ xs
        A[:, :, t // 3, t % 3] = df.abs().t() @ xs.abs()
    return dW, df.sum(0), A, df.abs().sum(0)


def pool_ref(c, last=False):
    """max_pool2d(3, 2, 1) of c [N, H, W, C] over the 9 window positions in scan order with a
    strict > (the first maximum; last=True: the last one, the mutant): (values, window byte 0..8).
    Out-of-map positions never win: the centre (2 oy, 2 ox) is always inside."""
    c = c.double()
    n, H, W, C = c.shape
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    cp = F.pad(c, (0, 0, 1, 1, 1, 1), value=float("-inf"))
    best = torch.full((n, Ho, Wo, C), float("-inf"), dtype=torch.float64)
    idx = torch.zeros(n, Ho, Wo, C, dtype=torch.uint8)
    for t in range(9):
        ky, kx = t // 3, t % 3
        v = cp[:, ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2]
        upd = ((v >= best) & (v > float("-inf"))) if last else (v > best)
        best = torch.where(upd, v, best)
        idx = torch.where(upd, torch.full_like(idx, t), idx)
    return best, idx


def pool_bwd_ref(dp, idx, H, W):
    """The scatter-add: dc[n, 2 oy - 1 + ky, 2 ox - 1 + kx, c] += dp[n, oy, ox, c] for the
    window byte ky * 3 + kx. Returns (dc, A, hits): A on |dp|, hits = windows that chose the cell."""
    dp = dp.double()
    n, Ho, Wo, C = dp.shape
    pad = [torch.zeros(n, 2 * Ho + 2, 2 * Wo + 2, C, dtype=torch.float64) for _ in range(3)]
    for t in range(9):
        ky, kx = t // 3, t % 3
        sel = (idx == t).double()
        for buf, v in zip(pad, (dp * sel, dp.abs() * sel, sel)):
            buf[:, ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2] += v
    for buf in pad:  # no byte may point outside the map
        assert float(buf[:, 0].abs().sum()) == 0 and float(buf[:, :, 0].abs().sum()) == 0
        assert float(buf[:, H + 1:].abs().sum()) == 0 and float(buf[:, :, W + 1:].abs().sum()) == 0
    return tuple(buf[:, 1:H + 1, 1:W + 1].contiguous() for buf in pad)


# ------------------------------------------------------------------ bounds
def bf16_bound(ref, A, n):
    """|y - ref| <= 2^-8 |ref| + n 2^-23 A for a bf16 output of n summed terms: one
    round-to-nearest store, plus twice the first-order fp32 bound of the sum in any order."""
    return U_BF16 * ref.abs() + n * U_SUM * A


def f32_bound(A, n):
    return n * U_SUM * A


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound; where the bound is zero the values must be equal (else inf)."""
    err = (got.double() - ref).abs()
    if not bool(torch.isfinite(err).all()):
        return float("inf")
    z = bound <= 0
    if bool((err[z] > 0).any()):
        return float("inf")
    if bool(z.all()):
        return 0.0
    return float((err[~z] / bound[~z]).max())


def _granule(t):
    """Smallest k with t * 2^k integral everywhere (operands of the exact case)."""
    t = t.double()
    for k in range(13):
        if bool((t * 2 ** k == (t * 2 ** k).round()).all()):
            return k
    raise AssertionError("operand is no small dyadic rational")


def assert_fp32_exact(A, *factors, plus=()):
    """Every partial sum is a multiple of 2^-k below max A (k: the granules of the product's
    factors added, or the largest granule of the terms added to it, bias and residual), so it is
    exact in fp32 in any order while max A < 2^(24 - k)."""
    k = max([sum(_granule(o) for o in factors)] + [_granule(o) for o in plus])
    assert float(A.max()) < 2.0 ** (24 - k), (float(A.max()), k)


def assert_bf16_exact(ref):
    assert torch.equal(ref, ref.bfloat16().double()), float(ref.abs().max())


def round_trunc_bf16(t):
    """fp64 -> bf16 by truncation of the fp32 bits (the mutant of the round-to-nearest store)."""
    b = t.float().contiguous().view(torch.int32) & ~0xFFFF
    return b.view(torch.float32).double()


# ------------------------------------------------------------------ case generators
class Case:
    """Operand generator of one kind ('exact' / 'round'), one torch.Generator per case."""

    def __init__(self, kind, seed):
        assert kind in ("exact", "round")
        self.kind = kind
        self.exact = kind == "exact"
        self.g = torch.Generator().manual_seed(seed)

    def ints(self, shape, lo=-2, hi=2):
        return torch.randint(lo, hi + 1, shape, generator=self.g).double()

    def acts(self, shape):
        """bf16 activations / gradients / residuals."""
        if self.exact:
            return self.ints(shape).bfloat16()
        return torch.randn(shape, generator=self.g).bfloat16()

    def weights(self, cout, cin):
        """fp32 master weights [cout, cin, 3, 3]."""
        shape = (cout, cin, 3, 3)
        if self.exact:
            v = torch.tensor([-1.0, -0.5, 0.5, 1.0])[torch.randint(0, 4, shape, generator=self.g)]
            return (v * (torch.rand(shape, generator=self.g) < 0.5)).float()
        return (torch.randn(shape, generator=self.g) * 0.2).float()

    def bias(self, cout):
        if self.exact:
            return (self.ints((cout,), -4, 4) / 2).float()
        return (torch.randn(cout, generator=self.g) * 0.1).float()

    def obs(self, n, H, W):
        """One-hot-per-group observation words [n, H*W] int32; the last two images (n >= 3) are
        an all-empty map and a map whose border cells are all occupied (interior empty)."""
        w = torch.zeros(n, H * W, dtype=torch.int64)
        for off, k in PLANE_GROUPS:
            w |= 1 << (off + torch.randint(0, k, (n, H * W), generator=self.g))
        if n >= 3:
            w[n - 2] = EMPTY_WORD
            ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
            border = ((ys == 0) | (ys == H - 1) | (xs == 0) | (xs == W - 1)).reshape(-1)
            occupied = torch.where(w[n - 1] == EMPTY_WORD, torch.full_like(w[n - 1], EMPTY_WORD ^ 3),
                                   w[n - 1])
            w[n - 1] = torch.where(border, occupied, torch.full_like(occupied, EMPTY_WORD))
        return w.to(torch.int32)
