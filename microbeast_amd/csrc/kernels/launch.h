// Host-side launch geometry shared by the kernels' launchers: how many workgroups the device
// keeps resident for a kernel, and how large a weight gradient's partial-row buffer is. A
// kernel's *_parts query and its launch size their grid through the same calls here, so the
// partial rows one counts are the rows the other writes.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace mbk {

// multiprocessors of the current device, cached for the first device seen (every translation
// unit of the library shares this one cache); 256 where the query fails
inline int cu_count() {
  static const int cus = [] {
    int dev = 0, n = 0;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev);
    return n > 0 ? n : 256;
  }();
  return cus;
}

// workgroups of (kernel, threads, dynamic LDS) one CU holds, >= 1; raises the kernel's
// dynamic-LDS limit where the launch will need it. One occupancy query per call: a launcher
// on the hot path keeps the result in a static.
inline int blocks_per_cu(const void* kfn, int threads, size_t smem) {
  if (smem > 64 * 1024)
    (void)hipFuncSetAttribute(kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
  int per = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, kfn, threads, smem) != hipSuccess ||
      per < 1)
    per = 1;
  return per;
}

// resident workgroups of the whole device under a per-CU cap (occ: mbk_occ_f / mbk_occ_b of
// common.h, or null for none); the caps can change between calls, so they apply to a cached
// per-CU count too
inline int resident_blocks(int per_cu, int (*occ)(int)) {
  return cu_count() * (occ ? occ(per_cu) : per_cu);
}
inline int resident_blocks(const void* kfn, int threads, size_t smem, int (*occ)(int)) {
  return resident_blocks(blocks_per_cu(kfn, threads, smem), occ);
}

// The tile kernels split a tile-local pixel index in [0, imgs*H*W) into (image, y, x) with
// float reciprocals (tile.h PixSplit), exact while imgs*H*W < 2^22; every launcher of such a
// kernel checks its round here
inline bool index_math_ok(int imgs, int H, int W) {
  return H > 0 && W > 0 && H * W <= 1024 && (int64_t)imgs * H * W < (int64_t(1) << 22);
}

// ------------------------------------------------------------------ weight-gradient rows
// A conv layer's weight gradient leaves its kernel as nparts fp32 partial rows of
// [cout][9][cin] weights + [cout] biases; the reduce (conv.hip) sums them kReducePps rows per
// split and stages the split sums in scratch rows after the partial rows.
constexpr int kReducePps = 32;
constexpr int wgrad_row_floats(int cin, int cout) { return cout * 9 * cin + cout; }
constexpr int wgrad_reduce_splits(int nparts) { return (nparts + kReducePps - 1) / kReducePps; }
// floats of one layer's buffer: the rows, then the scratch rows
constexpr int64_t wgrad_partial_floats(int nparts, int cin, int cout) {
  return (int64_t)(nparts + wgrad_reduce_splits(nparts)) * wgrad_row_floats(cin, cout);
}

}  // namespace mbk
