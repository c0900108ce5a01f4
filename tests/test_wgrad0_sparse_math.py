"""The stage-0 weight gradient split into an empty-cell term and a sum over the non-empty cells
(conv.hip wgrad0_sparse_kernel), in float64 against autograd.

X = E + D with E the empty word in every in-map cell and D = X - E (zero except at the listed
cells, entries in {-1, 0, +1}). The weight gradient is linear in X, so for tap t with offset
off_t

    dW[t][ci][co] = E[ci] * S_t[co] + sum_{q listed} D[q][ci] * dY[q - off_t][co]
    S_t[co]       = sum_{p in map, p + off_t in map} dY[p][co]       (S_4 = the bias gradient)

for any observation and any E: a cell whose word differs from E is simply listed.
"""
import pytest
import torch
import torch.nn.functional as F

from microbeast_amd.ops.encoder import EMPTY_WORD, PLANE_GROUPS

H = W = 16
PLANES = 27
COUT = 16


def _planes(words):  # [H*W] int64 words -> [PLANES, H, W] float64 0 / 1
    b = (words.view(H, W, 1) >> torch.arange(PLANES)) & 1
    return b.permute(2, 0, 1).to(torch.float64)


def _random_words(g, n):
    w = torch.zeros(n, dtype=torch.int64)
    for off, k in PLANE_GROUPS:
        w |= 1 << (off + torch.randint(0, k, (n,), generator=g))
    return w


def _autograd(x, dy):
    w = torch.zeros(COUT, PLANES, 3, 3, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(COUT, dtype=torch.float64, requires_grad=True)
    F.conv2d(x[None], w, b, padding=1).backward(dy[None])
    return w.grad, b.grad


def _decomposed(words, dy, empty):
    """(dW [COUT, PLANES, 3, 3], db [COUT]) by the formula above, the non-empty cells listed in
    ascending order as the kernel does."""
    e = ((empty >> torch.arange(PLANES)) & 1).to(torch.float64)
    dyh = F.pad(dy, (1, 1, 1, 1))  # zero halo: dY outside the map
    dw = torch.zeros(COUT, PLANES, 3, 3, dtype=torch.float64)
    listed = [q for q in range(H * W) if int(words[q]) != empty]
    for ky in range(3):
        for kx in range(3):
            oy, ox = ky - 1, kx - 1
            ys = slice(max(0, -oy), H - max(0, oy))
            xs = slice(max(0, -ox), W - max(0, ox))
            s_t = dy[:, ys, xs].sum((1, 2))
            dw[:, :, ky, kx] = s_t[:, None] * e[None, :]
            for q in listed:
                y, x = divmod(q, W)
                d = (((int(words[q]) >> torch.arange(PLANES)) & 1).to(torch.float64) - e)
                dw[:, :, ky, kx] += dyh[:, y - oy + 1, x - ox + 1][:, None] * d[None, :]
    return dw, dy.sum((1, 2)), len(listed)


def _cases():
    g = torch.Generator().manual_seed(11)
    empty = torch.full((H * W,), EMPTY_WORD, dtype=torch.int64)
    border = empty.clone()
    cells = [0, W - 1, (H - 1) * W, H * W - 1,       # the four corners
             5, (H - 1) * W + 9, 7 * W, 4 * W + W - 1,  # top, bottom, left, right edges
             3 * W + 3]
    border[cells] = _random_words(g, len(cells))
    return {"empty": (empty, 0), "border": (border, None),
            "random": (_random_words(g, H * W), None)}


@pytest.mark.parametrize("case", ["empty", "border", "random"])
def test_decomposition_equals_autograd(case):
    words, nlisted = _cases()[case]
    dy = torch.randn(COUT, H, W, dtype=torch.float64,
                     generator=torch.Generator().manual_seed(3))
    dw, db, n = _decomposed(words, dy, EMPTY_WORD)
    if nlisted is not None:
        assert n == nlisted
    rw, rb = _autograd(_planes(words), dy)
    assert float(rw.abs().sum()) > 0
    torch.testing.assert_close(dw, rw, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(db, rb, rtol=1e-12, atol=1e-12)


def test_identity_holds_for_a_wrong_empty_word():
    words, _ = _cases()["border"]
    dy = torch.randn(COUT, H, W, dtype=torch.float64,
                     generator=torch.Generator().manual_seed(4))
    wrong = (1 << 3) | (1 << 7) | (1 << 26)
    dw, db, n = _decomposed(words, dy, wrong)
    assert n == H * W  # every cell differs from it, so every cell is listed
    rw, rb = _autograd(_planes(words), dy)
    torch.testing.assert_close(dw, rw, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(db, rb, rtol=1e-12, atol=1e-12)


def test_empty_word_is_the_first_plane_of_every_group():
    assert EMPTY_WORD == 0x202421
    assert sum(k for _, k in PLANE_GROUPS) == PLANES
