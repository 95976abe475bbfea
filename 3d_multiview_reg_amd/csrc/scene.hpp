// What the kernels over a batch of scenes share (sync.hip's sync_kernel, posegraph.hip's posegraph_kernel; DESIGN.md
// 4.31): a scene is an edge list R_pair, t_pair, ij, w of n_edges edges over n_frags fragments with an anchor, one
// workgroup per scene.  Here: which edges count, the anchor's component, and the host's argument rules.  Integer and
// control logic only, inlined into each kernel; the workspace words, the treatment of an invalid scene and the LDS
// (sMem [N], sFlag [2]) stay the caller's.
#pragma once
#include "common.hpp"
#include "mvreg.h"
#include <math.h>

namespace mvr {

// w0[e] <- the weight of edge e (1 without `win`), or -1 for an edge that is ignored: an endpoint outside [0, N), a
// self-loop, a weight that is not finite or negative, a value of R_pair or t_pair that is not finite, or more(e)
// false (the caller's own per-edge rule, compiled in).  An ignored edge ORs 4 into sFlag[0], which the caller has
// cleared.  Thread e % kThreads owns edge e, here and in every later per-edge pass.  Ends with a barrier.
template <int kThreads, class More>
__device__ __forceinline__ void scene_edge_test(const double* Rp, const double* tp, const int32_t* ij,
                                                const double* win, int N, int E, double* w0, int* sFlag, More more) {
  int ign = 0;
  for (int e = threadIdx.x; e < E; e += kThreads) {
    const int i = ij[2 * e], j = ij[2 * e + 1];
    const double wv = win ? win[e] : 1.0;
    bool ok = i >= 0 && i < N && j >= 0 && j < N && i != j && isfinite(wv) && wv >= 0.0;
    for (int q = 0; q < 9; ++q) ok = ok && isfinite(Rp[(int64_t)9 * e + q]);
    for (int q = 0; q < 3; ++q) ok = ok && isfinite(tp[(int64_t)3 * e + q]);
    ok = ok && more(e);
    w0[e] = ok ? wv : -1.0;
    ign |= !ok;
  }
  if (ign) atomicOr(&sFlag[0], 4);
  __syncthreads();
}

// The anchor's component over the edges with w0 > 0, grown on sMem (the caller has set sMem[f] = (f == anchor) and
// passed a barrier) in at most N + 1 rounds; sFlag[1] is the rounds' change flag.  Several threads may store the same
// 1 in a round: plain stores, no atomics.  Then a counted edge whose source is no member gets w0 = 0.  Returns the
// member count, valid in every thread; the caller's barrier follows its own pass over w0.
template <int kThreads>
__device__ __forceinline__ int scene_component(const int32_t* ij, int N, int E, double* w0, int* sMem, int* sFlag) {
  const int tid = threadIdx.x;
  for (int round = 0; round <= N; ++round) {
    if (tid == 0) sFlag[1] = 0;
    __syncthreads();
    for (int e = tid; e < E; e += kThreads)
      if (w0[e] > 0.0) {
        const int i = ij[2 * e], j = ij[2 * e + 1];
        if (sMem[i] != sMem[j]) { sMem[i] = 1; sMem[j] = 1; sFlag[1] = 1; }
      }
    __syncthreads();
    const int changed = sFlag[1];
    __syncthreads();
    if (!changed) break;
  }
  int Nm = 0;
  for (int f = 0; f < N; ++f) Nm += sMem[f];
  for (int e = tid; e < E; e += kThreads)
    if (w0[e] > 0.0 && !sMem[ij[2 * e]]) w0[e] = 0.0;
  return Nm;
}

// ---- the host entries' argument rules
// the counts: a batch of S scenes of at most max_frags <= MVR_SYNC_MAX_FRAGS fragments and max_edges edges
static inline bool scene_counts_ok(int S, int max_frags, int max_edges, int anchor) {
  return S >= 0 && max_frags >= 0 && max_edges >= 0 && max_frags <= MVR_SYNC_MAX_FRAGS && anchor >= 0 &&
         (max_frags == 0 || anchor < max_frags);
}

// the scene strides of a batch, and a workspace of `need` bytes aligned for doubles
static inline bool scene_buffers_ok(int S, int max_frags, int max_edges, int64_t e_sstride, int64_t f_sstride,
                                    const void* workspace, size_t workspace_bytes, size_t need) {
  if (S > 1 && (e_sstride < max_edges || f_sstride < max_frags)) return false;
  return workspace && workspace_bytes >= need && !(reinterpret_cast<uintptr_t>(workspace) & 7);
}

}  // namespace mvr
