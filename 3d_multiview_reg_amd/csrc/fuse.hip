// Scene fusion (mvr_fuse_scene): the registered fragments of a scene mapped by their poses into one frame and merged
// per voxel — Open3D's `pcd_combined += pcd.transform(pose)` followed by voxel_down_sample, restated (mvreg.h).
//   1. every member point is mapped in fp64 (q, and the rotated normal, kept in the workspace) while each workgroup
//      reduces the minimum of its points; one workgroup folds the partial minima into the grid origin lo = min - voxel / 2;
//   2. voxel index floor((q - lo) / voxel) per axis (the expression of overlap.hip's voxel_key_kernel), 21 bits per
//      axis in one 64-bit key; points of fragments left out get a key above every voxel's;
//   3. the in-tree stable radix sort (radix.hip), head flags, their exclusive scan and the runs' first rows;
//   4. one thread per occupied voxel walks its run in sorted (= input) order: fp64 sums, counts, fragment changes
//      (eight points' rows fetched ahead of the fold).
// No floating-point atomics anywhere: a minimum is exact in any order and every sum is one thread's left fold.
// Gather / latency bound (24-byte rows fetched through the sort's permutation).
#include "common.hpp"
#include "prof.hpp"
#include "radix.hpp"
#include "rindex.hpp"
#include "mvreg.h"

namespace mvr {
namespace {

constexpr int FU_BITS = 21;                              // bits per voxel coordinate
constexpr double FU_LIMIT = (double)(1 << FU_BITS);      // voxel indices lie in [0, 2^21)
constexpr uint64_t FU_OUT = 1ull << 63;                  // key of a point that is not fused: after every voxel
constexpr int FU_MIN_BLOCKS = 1024;                      // workgroups (and partial minima) of the transform pass

struct FuseCtl {      // the call's device scalars (workspace)
  double lo[3];       // grid origin
  int32_t bad;        // a non-finite mapped point, or a voxel index outside the key
  int32_t n_voxels;
};

__device__ __forceinline__ int frag_of(const int64_t* off, int B, int64_t i) {
  int lo = 0, hi = B;   // off[lo] <= i < off[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (off[mid] <= i) lo = mid; else hi = mid;
  }
  return lo;
}

// q = R x + t of every member point and, with normals, R n (both kept for the later passes), its fragment (-1: left
// out), and the workgroup's minimum per axis.  A non-finite q is recorded in pbad: fmin would drop a NaN silently.
__global__ void fuse_transform_kernel(const double* __restrict__ xyz, const double* __restrict__ normals,
                                      const int64_t* __restrict__ off, int B, int64_t M,
                                      const double* __restrict__ poses, const uint8_t* __restrict__ member,
                                      double* __restrict__ q, double* __restrict__ qn, int32_t* __restrict__ frag,
                                      double* __restrict__ pmin, int32_t* __restrict__ pbad) {
  __shared__ double red[3][256];
  __shared__ int redb[256];
  double m[3] = {1e300, 1e300, 1e300};
  int bad = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < M; i += (int64_t)gridDim.x * blockDim.x) {
    const int b = frag_of(off, B, i);
    if (member && !member[b]) {
      frag[i] = -1;
      continue;
    }
    const double* T = poses + 12 * (int64_t)b;
    const double x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
    const double p[3] = {T[0] * x + T[1] * y + T[2] * z + T[3], T[4] * x + T[5] * y + T[6] * z + T[7],
                         T[8] * x + T[9] * y + T[10] * z + T[11]};
    frag[i] = b;
    for (int d = 0; d < 3; ++d) {
      q[3 * i + d] = p[d];
      m[d] = fmin(m[d], p[d]);
      if (!isfinite(p[d])) bad = 1;
    }
    if (normals) {
      const double nx = normals[3 * i], ny = normals[3 * i + 1], nz = normals[3 * i + 2];
      qn[3 * i] = T[0] * nx + T[1] * ny + T[2] * nz;
      qn[3 * i + 1] = T[4] * nx + T[5] * ny + T[6] * nz;
      qn[3 * i + 2] = T[8] * nx + T[9] * ny + T[10] * nz;
    }
  }
  for (int d = 0; d < 3; ++d) red[d][threadIdx.x] = m[d];
  redb[threadIdx.x] = bad;
  __syncthreads();
  for (int s = blockDim.x / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      for (int d = 0; d < 3; ++d) red[d][threadIdx.x] = fmin(red[d][threadIdx.x], red[d][threadIdx.x + s]);
      redb[threadIdx.x] |= redb[threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x < 3) pmin[3 * blockIdx.x + threadIdx.x] = red[threadIdx.x][0];
  if (threadIdx.x == 3) pbad[blockIdx.x] = redb[0];
}

// one workgroup: the partial minima -> the grid origin (Open3D: min_bound - voxel / 2)
__global__ void fuse_origin_kernel(const double* __restrict__ pmin, const int32_t* __restrict__ pbad, int nblk,
                                   double v, FuseCtl* ctl) {
  __shared__ double red[3][256];
  __shared__ int redb[256];
  double m[3] = {1e300, 1e300, 1e300};
  int bad = 0;
  for (int i = threadIdx.x; i < nblk; i += blockDim.x) {
    for (int d = 0; d < 3; ++d) m[d] = fmin(m[d], pmin[3 * i + d]);
    bad |= pbad[i];
  }
  for (int d = 0; d < 3; ++d) red[d][threadIdx.x] = m[d];
  redb[threadIdx.x] = bad;
  __syncthreads();
  for (int s = blockDim.x / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      for (int d = 0; d < 3; ++d) red[d][threadIdx.x] = fmin(red[d][threadIdx.x], red[d][threadIdx.x + s]);
      redb[threadIdx.x] |= redb[threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x < 3) ctl->lo[threadIdx.x] = red[threadIdx.x][0] - v * 0.5;
  if (threadIdx.x == 3) {
    ctl->bad = redb[0];
    ctl->n_voxels = 0;
  }
}

// The fp64 quotient is tested before the cast: an index that does not fit its 21 bits (or a NaN) marks the call
// (the same value from every writer) and the point gets the key of the points left out.
__global__ void fuse_key_kernel(const double* __restrict__ q, const int32_t* __restrict__ frag, int64_t M, double v,
                                FuseCtl* ctl, uint64_t* keys, uint64_t* keys2, int32_t* idx) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M) return;
  uint64_t k = FU_OUT;
  if (frag[i] >= 0) {
    double f[3];
    bool ok = true;
    for (int d = 0; d < 3; ++d) {
      f[d] = floor((q[3 * i + d] - ctl->lo[d]) / v);
      ok = ok && f[d] >= 0.0 && f[d] < FU_LIMIT;
    }
    if (ok)
      k = ((uint64_t)(int64_t)f[0] << (2 * FU_BITS)) | ((uint64_t)(int64_t)f[1] << FU_BITS) | (uint64_t)(int64_t)f[2];
    else
      ctl->bad = 1;
  }
  keys[i] = k;
  keys2[i] = k;
  idx[i] = (int32_t)i;
}

// sorted keys from the sort's permutation (the sort itself returns the values only)
__global__ void fuse_gather_keys_kernel(const uint64_t* __restrict__ k, const int32_t* __restrict__ perm, int64_t n,
                                        uint64_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = k[perm[i]];
}

// the points left out form one last run of their own (key FU_OUT): its head ends the last voxel's run
__global__ void fuse_head_kernel(const uint64_t* __restrict__ k, int64_t n, int32_t* head) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  head[i] = (i == 0 || k[i] != k[i - 1]) ? 1 : 0;
}

// start[o] = first sorted row of run o; start has n + 1 entries
__global__ void fuse_starts_kernel(const int32_t* __restrict__ head, const int32_t* __restrict__ pos, int64_t n,
                                   int32_t* __restrict__ start) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && head[i]) start[pos[i]] = (int32_t)i;
}

__global__ void fuse_count_kernel(const uint64_t* __restrict__ k, const int32_t* __restrict__ head,
                                  const int32_t* __restrict__ pos, int64_t n, int32_t* start, FuseCtl* ctl,
                                  int64_t* out_count) {
  const int32_t runs = pos[n - 1] + head[n - 1];
  const int32_t nv = runs - (k[n - 1] == FU_OUT ? 1 : 0);
  start[runs] = (int32_t)n;     // the end of the last run (runs <= n)
  ctl->n_voxels = nv;
  *out_count = ctl->bad ? -1 : (int64_t)nv;
}

__global__ void fuse_zero_count_kernel(int64_t* out_count) { *out_count = 0; }

// One thread per occupied voxel (rows of the output, so every lane of a wave has a run): a left fold over the
// run's points in sorted order, which the stable sort keeps equal to input order (ascending fragment, then row).
// A point costs two dependent gathers (the permutation, then its rows), and a wave lasts as long as its longest
// run: the rows of FU_AHEAD points are fetched together before they are folded one after the other, which divides
// the chain of latencies by FU_AHEAD and leaves the order of the sums alone.  Past the end of the run the last row
// is fetched again and +0.0 is added (no sum here is ever -0.0, so that changes no bit) and its fragment repeats:
// straight-line code, which keeps the loads ahead of the fold.
constexpr int FU_AHEAD = 8;
template <bool NORMALS>
__global__ void __launch_bounds__(256)
fuse_run_kernel(const double* __restrict__ q, const double* __restrict__ qn, const int32_t* __restrict__ frag,
                const int32_t* __restrict__ sidx, const int32_t* __restrict__ start, const FuseCtl* __restrict__ ctl,
                double* __restrict__ out_xyz, double* __restrict__ out_normals, int32_t* __restrict__ out_np,
                int32_t* __restrict__ out_nf) {
  const int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= (int64_t)ctl->n_voxels) return;
  const int32_t j0 = start[o], j1 = start[o + 1];
  double s[3] = {0.0, 0.0, 0.0}, sn[3] = {0.0, 0.0, 0.0};
  int nf = 0, last = -1;
  for (int32_t j = j0; j < j1; j += FU_AHEAD) {
    int64_t p[FU_AHEAD];
    double v[FU_AHEAD][3], n[FU_AHEAD][3];
    int b[FU_AHEAD];
#pragma unroll
    for (int u = 0; u < FU_AHEAD; ++u) p[u] = sidx[min(j + u, j1 - 1)];
#pragma unroll
    for (int u = 0; u < FU_AHEAD; ++u) {
      const bool in = j + u < j1;
      b[u] = frag[p[u]];
      for (int d = 0; d < 3; ++d) v[u][d] = in ? q[3 * p[u] + d] : 0.0;
      if (NORMALS)
        for (int d = 0; d < 3; ++d) n[u][d] = in ? qn[3 * p[u] + d] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < FU_AHEAD; ++u) {
      for (int d = 0; d < 3; ++d) s[d] += v[u][d];
      if (NORMALS)
        for (int d = 0; d < 3; ++d) sn[d] += n[u][d];
      nf += b[u] != last ? 1 : 0;
      last = b[u];
    }
  }
  const double cnt = (double)(j1 - j0);
  for (int d = 0; d < 3; ++d) out_xyz[3 * o + d] = s[d] / cnt;
  out_np[o] = j1 - j0;
  out_nf[o] = nf;
  if (NORMALS) {
    if (sn[0] == 0.0 && sn[1] == 0.0 && sn[2] == 0.0) {
      out_normals[3 * o] = 0.0;
      out_normals[3 * o + 1] = 0.0;
      out_normals[3 * o + 2] = 1.0;
    } else {
      const double len = sqrt(sn[0] * sn[0] + sn[1] * sn[1] + sn[2] * sn[2]);
      for (int d = 0; d < 3; ++d) out_normals[3 * o + d] = sn[d] / len;
    }
  }
}

inline unsigned nb(int64_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace
}  // namespace mvr

using namespace mvr;

extern "C" size_t mvr_fuse_scene_workspace_bytes(int64_t M) {
  const size_t m = (size_t)(M > 0 ? M : 1);
  // q, R n, fragment, keys (copy, sorted), permutation, head, pos, start, partial minima / flags, the scalars;
  // 256-byte alignment
  return m * (24 + 24 + 4 + 8 + 8 + 4 + 4 + 4) + (m + 1) * 4 + FU_MIN_BLOCKS * (24 + 4) + sizeof(FuseCtl) +
         radix_ws_bytes(M > 0 ? M : 1) + scan_ws_bytes(M > 0 ? M : 1) + 15 * 256;
}

extern "C" int mvr_fuse_scene(const double* xyz, const double* normals, const int64_t* off, int B, int64_t M,
                              const double* poses, const uint8_t* member, double voxel, void* ws, size_t ws_bytes,
                              double* out_xyz, double* out_normals, int32_t* out_n_points, int32_t* out_n_frags,
                              int64_t* out_count, hipStream_t s) {
  if (M < 0 || M > 0x7fffffff || B <= 0 || !(voxel > 0.0) || !out_count) return MVR_EINVAL;
  if (M > 0 && (!xyz || !off || !poses || !ws || !out_xyz || !out_n_points || !out_n_frags ||
                ws_bytes < mvr_fuse_scene_workspace_bytes(M) || (normals != nullptr) != (out_normals != nullptr)))
    return MVR_EINVAL;
  if (M == 0) {   // nothing to fuse (NULL point / workspace pointers allowed)
    hipLaunchKernelGGL(fuse_zero_count_kernel, dim3(1), dim3(1), 0, s, out_count);
    MVR_CHECK_LAUNCH();
    return MVR_OK;
  }
  // bytes the launches must move per point: the point in, q out and read back twice, keys and permutation through
  // 8 sort passes (24 each), the flag / scan / start arrays, the runs' gathers (normals included), the rows out
  ProfScope prof(PK_SPARSE_MISC, 0.0, (double)M * (normals ? 456.0 : 384.0), s);
  char* p = reinterpret_cast<char*>(ws);
  const size_t m = (size_t)M;
  double* q = reinterpret_cast<double*>(take(p, m * 24));
  double* qn = reinterpret_cast<double*>(take(p, m * 24));
  int32_t* frag = reinterpret_cast<int32_t*>(take(p, m * 4));
  uint64_t* kin = reinterpret_cast<uint64_t*>(take(p, m * 8));
  uint64_t* kout = reinterpret_cast<uint64_t*>(take(p, m * 8));
  int32_t* vout = reinterpret_cast<int32_t*>(take(p, m * 4));
  int32_t* head = reinterpret_cast<int32_t*>(take(p, m * 4));
  int32_t* pos = reinterpret_cast<int32_t*>(take(p, m * 4));
  int32_t* start = reinterpret_cast<int32_t*>(take(p, (m + 1) * 4));
  double* pmin = reinterpret_cast<double*>(take(p, FU_MIN_BLOCKS * 24));
  int32_t* pbad = reinterpret_cast<int32_t*>(take(p, FU_MIN_BLOCKS * 4));
  FuseCtl* ctl = reinterpret_cast<FuseCtl*>(take(p, sizeof(FuseCtl)));
  const size_t st = radix_ws_bytes(M), sc = scan_ws_bytes(M);
  void* tsort = take(p, st);
  void* tscan = take(p, sc);
  RadixWs rw = radix_ws(tsort, M);
  const int nblk = (int)std::min<int64_t>((M + 255) / 256, FU_MIN_BLOCKS);
  hipLaunchKernelGGL(fuse_transform_kernel, dim3(nblk), dim3(256), 0, s, xyz, normals, off, B, M, poses, member, q, qn,
                     frag, pmin, pbad);
  hipLaunchKernelGGL(fuse_origin_kernel, dim3(1), dim3(256), 0, s, pmin, pbad, nblk, voxel, ctl);
  hipLaunchKernelGGL(fuse_key_kernel, dim3(nb(M)), dim3(256), 0, s, q, frag, M, voxel, ctl, rw.ka, kin, rw.va);
  int rc = radix_sort(rw, 64, vout, s);   // stable: a voxel's points stay in input order
  if (rc != MVR_OK) return rc;
  hipLaunchKernelGGL(fuse_gather_keys_kernel, dim3(nb(M)), dim3(256), 0, s, kin, vout, M, kout);
  hipLaunchKernelGGL(fuse_head_kernel, dim3(nb(M)), dim3(256), 0, s, kout, M, head);
  if ((rc = excl_scan_i32(head, pos, M, tscan, sc, s)) != MVR_OK) return rc;
  hipLaunchKernelGGL(fuse_starts_kernel, dim3(nb(M)), dim3(256), 0, s, head, pos, M, start);
  hipLaunchKernelGGL(fuse_count_kernel, dim3(1), dim3(1), 0, s, kout, head, pos, M, start, ctl, out_count);
  if (normals)
    hipLaunchKernelGGL(fuse_run_kernel<true>, dim3(nb(M)), dim3(256), 0, s, q, qn, frag, vout, start, ctl, out_xyz,
                       out_normals, out_n_points, out_n_frags);
  else
    hipLaunchKernelGGL(fuse_run_kernel<false>, dim3(nb(M)), dim3(256), 0, s, q, qn, frag, vout, start, ctl, out_xyz,
                       out_normals, out_n_points, out_n_frags);
  MVR_CHECK_LAUNCH();
  return MVR_OK;
}
