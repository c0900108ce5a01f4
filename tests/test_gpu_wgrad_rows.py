"""The weight gradients' partial-row buffer contract (csrc/kernels/launch.h) and the batched
reduce that reads it (conv.hip mbk_wgrad_reduce_batch), called directly.

A layer's buffer is nparts rows of cout*9*cin + cout floats, then ceil(nparts / 32) scratch rows
for the two-level reduce (more than 64 rows). Every caller sizes its buffer by
mbk_wgrad_partial_floats, so the value is the contract: it is spelled out here, and the reduce
must stay inside it (a guard row after the buffer keeps its sentinel)."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

# (cin, cin_real, cout): the bit-plane stage-0 layer (27 real channels in 32) and the trunk's
SHAPES = ((32, 27, 16), (16, 16, 16), (16, 16, 32), (32, 32, 32))
# 64: the last single-level size; 65 and 130: two-level, with 3 and 5 scratch rows
NPARTS = (1, 64, 65, 130)
SENTINEL = float("nan")


def _bits(t):
    return t.view(torch.int32)


def _run(jobs):
    from microbeast_amd import _native as N
    from microbeast_amd.ops.encoder import _RJob
    arr = (_RJob * len(jobs))(*jobs)
    N.check(N.kernels().mbk_wgrad_reduce_batch(ctypes.cast(arr, ctypes.c_void_p), len(jobs),
                                               N.stream_ptr()), "wgrad_reduce_batch")


@pytest.mark.parametrize("nparts", NPARTS)
def test_reduce_batch_stays_inside_the_partial_row_contract(cuda, nparts):
    from microbeast_amd import _native as N
    from microbeast_amd.ops.encoder import _RJob
    k = N.kernels()
    g = torch.Generator().manual_seed(100 + nparts)
    scratch_rows = -(-nparts // 32)
    bufs, outs_a, outs_b, jobs_a, jobs_b = [], [], [], [], []
    for cin, cin_real, cout in SHAPES:
        row = cout * 9 * cin + cout
        need = k.mbk_wgrad_partial_floats(nparts, cin, cout)
        assert need == (nparts + scratch_rows) * row, (nparts, cin, cout)
        buf = torch.full((need + row,), SENTINEL, dtype=torch.float32)
        buf[:nparts * row] = torch.randn(nparts * row, generator=g)
        buf = buf.to(cuda)
        bufs.append(buf)
        for outs, jobs in ((outs_a, jobs_a), (outs_b, jobs_b)):
            dw = torch.full((cout, cin_real, 3, 3), SENTINEL, dtype=torch.float32, device=cuda)
            db = torch.full((cout,), SENTINEL, dtype=torch.float32, device=cuda)
            outs.append((dw, db))
            jobs.append(_RJob(buf.data_ptr(), dw.data_ptr(), db.data_ptr(), nparts, cin, cin_real,
                              cout))
    guards = [b[-(cout * 9 * cin + cout):].clone() for b, (cin, _, cout) in zip(bufs, SHAPES)]
    _run(jobs_a)                   # one batch holding all four layer shapes
    for j in jobs_b:               # four batches of one
        _run([j])
    torch.cuda.synchronize()
    for buf, guard, (dwa, dba), (dwb, dbb), (cin, cin_real, cout) in zip(bufs, guards, outs_a,
                                                                        outs_b, SHAPES):
        row = cout * 9 * cin + cout
        assert torch.equal(_bits(dwa), _bits(dwb)) and torch.equal(_bits(dba), _bits(dbb)), \
            f"batched vs single differ {(cin, cin_real, cout)}"
        assert torch.equal(_bits(buf[-row:]), _bits(guard)), \
            f"guard row written {(cin, cin_real, cout)}"
        rows = buf[:nparts * row].view(nparts, row).double().cpu()
        ref, mag = rows.sum(0), rows.abs().sum(0)

        def as_dw(v):  # row order [co][tap][ci] -> dw [co][ci < cin_real][tap]
            return v[:cout * 9 * cin].view(cout, 9, cin).permute(0, 2, 1)[:, :cin_real]

        # fp32 recursive summation of nparts terms, any order: |err| <= (n - 1) 2^-24 sum |x_i|
        u = (nparts - 1) * 2.0 ** -24
        err_w = (dwa.double().cpu().view(cout, cin_real, 9) - as_dw(ref)).abs()
        err_b = (dba.double().cpu() - ref[cout * 9 * cin:]).abs()
        print(f"nparts {nparts} {(cin, cin_real, cout)}: dw err/bound "
              f"{(err_w / (u * as_dw(mag)).clamp_min(1e-300)).max().item():.3g}, db err/bound "
              f"{(err_b / (u * mag[cout * 9 * cin:]).clamp_min(1e-300)).max().item():.3g}")
        assert bool((err_w <= u * as_dw(mag)).all()), f"dw {(cin, cin_real, cout)}"
        assert bool((err_b <= u * mag[cout * 9 * cin:]).all()), f"db {(cin, cin_real, cout)}"
