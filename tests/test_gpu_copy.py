"""copy.hip on the MI355X beyond freshly allocated tensors: ``multi_copy`` on its 16-byte, 4-byte
and byte paths, its tails, its grid-stride loop and the chunking above 16 segments;
``row_gather`` on both granules; the sparse-row I/O of the graph policy step on hand-built rows
(count clamp, out-of-range cells, refusals). Everything is exact, and every destination is a
slice of a larger sentinel-filled buffer whose other bytes must not change."""
import ctypes

import pytest
import torch

from microbeast_amd import _native as N
from microbeast_amd.ops.copy import MAX_SEGS, _Seg, multi_copy, row_gather

pytestmark = pytest.mark.gpu

HIP_ERROR_INVALID_VALUE = 1
SENT = 0xA5
OFFSETS = [(0, 0), (4, 8), (4, 4), (1, 1), (1, 2), (0, 3)]  # (src, dst) mod 16, in bytes
LENGTHS = [0, 1, 15, 16, 17, 4099, 2 * 1024 * 1024 + 19]    # the last: > 512 * 256 * 16 bytes


def _layout(lengths, offs):
    """Byte positions of one segment per length inside a shared buffer: each starts at a
    256-byte boundary plus ``off`` (a callable of the segment number), with a gap behind."""
    pos, at = [], 256
    for i, n in enumerate(lengths):
        pos.append(at + offs(i))
        at = (at + 16 + n + 64 + 255) // 256 * 256
    return pos, at + 256


def _copy_and_check(dev, lengths, src_off, dst_off, seed=0):
    sp, s_total = _layout(lengths, src_off)
    dp, d_total = _layout(lengths, dst_off)
    g = torch.Generator().manual_seed(seed)
    src_h = torch.randint(0, 256, (s_total,), generator=g, dtype=torch.uint8)
    src, dst = src_h.to(dev), torch.full((d_total,), SENT, dtype=torch.uint8, device=dev)
    assert src.data_ptr() % 256 == 0 and dst.data_ptr() % 256 == 0
    want = torch.full((d_total,), SENT, dtype=torch.uint8)
    pairs = []
    for n, a, b in zip(lengths, sp, dp):
        pairs.append((src[a:a + n], dst[b:b + n]))
        want[b:b + n] = src_h[a:a + n]
    multi_copy(pairs)
    torch.cuda.synchronize()
    assert torch.equal(dst.cpu(), want)
    assert torch.equal(src.cpu(), src_h)


@pytest.mark.parametrize("so,do", OFFSETS)
def test_multi_copy_alignments_and_lengths(cuda, so, do):
    """Every length at one (src, dst) misalignment, in ONE launch (so a 1-byte and a 2 MiB
    segment share a grid): (0,0) the 16-byte path, (4,8) / (4,4) the 4-byte path, the rest the
    byte path."""
    _copy_and_check(cuda, LENGTHS, lambda i: so, lambda i: do, seed=so * 16 + do)


@pytest.mark.parametrize("npairs", [17, 33])
def test_multi_copy_chunks_above_16_segments(cuda, npairs):
    assert npairs > MAX_SEGS
    lengths = [(37 * i) % 301 + (i % 3 == 0) * 4096 for i in range(npairs)]
    _copy_and_check(cuda, lengths, lambda i: OFFSETS[i % 6][0], lambda i: OFFSETS[i % 6][1],
                    seed=npairs)


def test_multi_copy_refuses_17_segments_and_accepts_none(cuda):
    src = torch.arange(64, dtype=torch.uint8, device=cuda)
    dst = torch.full((64,), SENT, dtype=torch.uint8, device=cuda)
    arr = (_Seg * 17)()
    for j in range(17):
        arr[j] = _Seg(src.data_ptr(), dst.data_ptr(), 64)
    k = N.kernels()
    p = ctypes.cast(arr, ctypes.c_void_p)
    assert k.mbk_multi_copy(p, 17, N.stream_ptr()) == HIP_ERROR_INVALID_VALUE
    assert k.mbk_multi_copy(p, 0, N.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert bool((dst.cpu() == SENT).all())  # neither call launched anything
    assert k.mbk_multi_copy(p, 16, N.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert torch.equal(dst, src)


def _gather_and_check(dev, src, idx, k, lead=64):
    """row_gather into a slice ``lead`` elements inside a sentinel buffer."""
    row = src[0].numel()
    sent = -1515870811 if src.dtype == torch.int32 else -23131  # 0xA5A5...
    buf = torch.full((2 * lead + max(k, 1) * row,), sent, dtype=src.dtype, device=dev)
    out = buf[lead:lead + k * row].view(k, row)
    idx_d = torch.tensor(idx, dtype=torch.int64, device=dev)
    got = row_gather(src, idx_d, k, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr() or k == 0
    want = torch.full_like(buf, sent).cpu()
    if k:
        want[lead:lead + k * row] = src.cpu()[torch.tensor(idx[:k])].reshape(-1)
    assert torch.equal(buf.cpu(), want)


@pytest.mark.parametrize("row_bytes", [4, 36, 64, 1168, 256 * 1024 + 16])
def test_row_gather(cuda, row_bytes):
    """4 / 36: 4-byte granules; 64 / 1168: 16-byte granules; 256 KiB + 16: more than 64 * 256
    granules per row, so every thread loops. Repeated indices, and k below len(idx)."""
    R, nv = 9, row_bytes // 4
    g = torch.Generator().manual_seed(row_bytes)
    src = torch.randint(-2 ** 31, 2 ** 31 - 1, (R, nv), generator=g, dtype=torch.int64)
    src = src.to(torch.int32).to(cuda)
    assert src.data_ptr() % 16 == 0
    idx = [8, 0, 3, 3, 7, 0, 8, 1, 2, 5, 4]
    _gather_and_check(cuda, src, idx, 7)
    _gather_and_check(cuda, src, idx, len(idx))
    _gather_and_check(cuda, src, idx, 1)
    _gather_and_check(cuda, src, idx, 0)  # k = 0: out untouched
    # 16-byte rows into a destination that is only 4-byte aligned: the 4-byte granules
    if row_bytes % 16 == 0:
        _gather_and_check(cuda, src, idx, 7, lead=61)


def test_row_gather_unaligned_source_view(cuda):
    """A 64-byte-row source that starts 4 bytes into its allocation falls back to 4-byte
    granules (a 16-byte load there would be misaligned)."""
    R, nv = 9, 16
    base = torch.arange(1 + R * nv + 3, dtype=torch.int32, device=cuda) * 7 + 1
    src = base[1:1 + R * nv].view(R, nv)
    assert src.data_ptr() % 16 == 4 and src.is_contiguous()
    _gather_and_check(cuda, src, [8, 0, 3, 3, 7, 0, 8, 1], 6)


def test_row_gather_refuses_rows_that_are_no_multiple_of_4_bytes(cuda):
    src = torch.arange(27, dtype=torch.int16, device=cuda).view(9, 3)  # 6-byte rows
    out = torch.full((4, 3), -23131, dtype=torch.int16, device=cuda)
    idx = torch.tensor([1, 2, 3, 4], dtype=torch.int64, device=cuda)
    with pytest.raises(RuntimeError, match="row_gather"):
        row_gather(src, idx, 4, out=out)
    torch.cuda.synchronize()
    assert bool((out.cpu() == -23131).all())


# --- sparse-row I/O on hand-built rows (beside test_gpu_act.py::test_graph_sparse_row_io) ---

def _word(lo, hi):
    """uint32 lo | hi << 16 as the int32 that holds the same bits"""
    w = (lo & 0xFFFF) | ((hi & 0xFFFF) << 16)
    return w - (1 << 32) if w >= (1 << 31) else w


def _build_rows(S, E, stride, seed):
    """E hand-built rows and the dense codes / resources they must expand to. Row kinds:
    0: count field S + 3 (clamped to S): S - 2 real entries and two with a cell index >= S
       (dropped) in positions 1..S, then words past position S that name cells no real entry
       covers -- reading them would show;
    1: count 0 (the entries behind it are stale and must be ignored);
    2: all S cells occupied, in a shuffled order;
    3: a few entries, some with cell index S, S + 1 and 0xFFFF (dropped);
    4: a sparse ordinary row."""
    g = torch.Generator().manual_seed(seed)
    rows = torch.full((E, stride), _word(0, 0x7777), dtype=torch.int32)  # stale: cell 0, code 0x7777
    codes = torch.zeros(E, S, dtype=torch.int64)
    res = torch.zeros(E, dtype=torch.int32)
    code = lambda: int(torch.randint(1, 0x10000, (1,), generator=g))  # noqa: E731
    for e in range(E):
        kind = e % 5
        perm = torch.randperm(S, generator=g).tolist()
        r = int(torch.randint(0, 0x10000, (1,), generator=g))
        res[e] = r
        ent = []
        if kind == 0:
            covered, free = perm[:S - 2], perm[S - 2:]
            ent = [(c, code()) for c in covered]
            ent.insert(S // 3, (S, code()))
            ent.insert(2 * S // 3, (0xFFFF, code()))
            assert len(ent) == S
            count = S + 3
            for q in range(S + 1, stride):  # never read: n is clamped to S
                rows[e, q] = _word(free[(q - S - 1) % 2], 0x5555)
        elif kind == 1:
            count = 0
        elif kind == 2:
            ent = [(c, code()) for c in perm]
            count = S
        elif kind == 3:
            ent = [(perm[0], code()), (S, code()), (perm[1], code()), (S + 1, code()),
                   (0xFFFF, code()), (perm[2], code())]
            count = len(ent)
        else:
            ent = [(c, code()) for c in perm[:max(1, S // 10)]]
            count = len(ent)
        rows[e, 0] = _word(count, r)
        for q, (c, v) in enumerate(ent):
            rows[e, 1 + q] = _word(c, v)
            if c < S:
                codes[e, c] = v
    return rows, codes, res


@pytest.mark.parametrize("E", [1, 5])
@pytest.mark.parametrize("S", [64, 100, 1024])
def test_rows_to_codes_hand_built_rows(cuda, S, E):
    stride = S + 4
    rows, want_codes, want_res = _build_rows(S, E, stride, seed=S + E)
    want16 = (want_codes - (want_codes >= 0x8000) * 0x10000).to(torch.int16)
    lead = 96
    buf = torch.full((2 * lead + E * S,), -23131, dtype=torch.int16, device=cuda)
    rbuf = torch.full((E + 16,), -7, dtype=torch.int32, device=cuda)
    rows_p = rows.pin_memory()
    N.check(N.kernels().mbk_rows_to_codes(rows_p.data_ptr(), stride, E, S, buf[lead:].data_ptr(),
                                          rbuf[8:].data_ptr(), N.stream_ptr()), "rows_to_codes")
    torch.cuda.synchronize()
    b, r = buf.cpu(), rbuf.cpu()
    assert torch.equal(b[lead:lead + E * S].view(E, S), want16)
    assert bool((b[:lead] == -23131).all()) and bool((b[lead + E * S:] == -23131).all())
    assert torch.equal(r[8:8 + E], want_res)  # the high half of word 0
    assert bool((r[:8] == -7).all()) and bool((r[8 + E:] == -7).all())
    assert torch.equal(rows_p, rows)  # the rows are only read


def test_sparse_row_io_refusals(cuda):
    k = N.kernels()
    st = N.stream_ptr()
    rows = torch.zeros(2, 1032, dtype=torch.int32, device=cuda)
    codes = torch.full((2, 1032), -23131, dtype=torch.int16, device=cuda)
    res = torch.full((2,), -7, dtype=torch.int32, device=cuda)
    a = (rows.data_ptr(),)
    z = (codes.data_ptr(), res.data_ptr(), st)
    assert k.mbk_rows_to_codes(*a, 1032, 2, 1025, *z) == HIP_ERROR_INVALID_VALUE  # S > 1024
    assert k.mbk_rows_to_codes(*a, 64, 2, 64, *z) == HIP_ERROR_INVALID_VALUE      # stride = S
    assert k.mbk_rows_to_codes(*a, 1, 0, 64, *z) == 0                              # E = 0
    assert k.mbk_codes_to_rows(codes.data_ptr(), 2, 64, rows.data_ptr(), 64, st) \
        == HIP_ERROR_INVALID_VALUE                                                 # stride = S
    assert k.mbk_codes_to_rows(codes.data_ptr(), 0, 64, rows.data_ptr(), 1, st) == 0
    torch.cuda.synchronize()
    assert bool((codes.cpu() == -23131).all()) and bool((res.cpu() == -7).all())
    assert int(rows.cpu().abs().sum()) == 0
    assert k.mbk_rows_to_codes(*a, 1025, 2, 1024, *z) == 0  # the largest accepted S
    torch.cuda.synchronize()
    assert int(codes.view(-1)[:2048].cpu().abs().sum()) == 0 and res.cpu().tolist() == [0, 0]


@pytest.mark.parametrize("S", [64, 100, 1024])
def test_codes_to_rows_all_cells_occupied(cuda, S):
    """Every cell non-zero with stride exactly S + 1: each row is filled to its last word and
    nothing lands behind it. (Env 3 is empty and env 4 sparse, so the count is not a constant.)"""
    E, stride = 5, S + 1
    g = torch.Generator().manual_seed(S)
    act = torch.randint(1, 0x10000, (E, S), generator=g, dtype=torch.int64)
    act[3] = 0
    act[4, torch.rand(S, generator=g) < 0.9] = 0
    act16 = (act - (act >= 0x8000) * 0x10000).to(torch.int16)
    lead = 32
    buf = torch.full((2 * lead + E * stride,), -7, dtype=torch.int32, device=cuda)
    act_d = act16.to(cuda)
    N.check(N.kernels().mbk_codes_to_rows(act_d.data_ptr(), E, S, buf[lead:].data_ptr(), stride,
                                          N.stream_ptr()), "codes_to_rows")
    torch.cuda.synchronize()
    want = torch.full((2 * lead + E * stride,), -7, dtype=torch.int32)
    for e in range(E):
        cells = act[e].nonzero().flatten().tolist()
        o = lead + e * stride
        want[o] = len(cells)
        for q, c in enumerate(cells):
            want[o + 1 + q] = _word(c, int(act[e, c]))
    assert int(want[lead]) == S and int(want[lead + 3 * stride]) == 0
    assert torch.equal(buf.cpu(), want)
