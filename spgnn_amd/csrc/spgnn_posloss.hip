// spgnn_posloss.hip — gfx950 (MI355X / CDNA4) auxiliary losses on the position stream of the SPGNN training step
// (reference job_runner.py:1827-1865 dist_pos_loss, switched on by USE_DIST_LOSS at job_runner.py:1901-1903):
//
//   d = mean_t  mean_{i,j in t} smooth_l1(A_ij, T_ij),  A_ij = exp(-sum_k |p_ik - p_jk|),  T_ij = exp(-hops_ij / diam_t)
//   c = mean_t  sum_{L present in t} || p[last node of label L] - M[L-1] ||^2          (0 while M is unset)
//   M <- mean_t S[t]  (first step)  |  0.15 M + 0.85 mean_t S[t],   S[t, L-1] = p[last node of L] or uniform noise
//
// Three kernels:
//   pos_tables   once per loader batch, one workgroup per tree: BFS from the tree's first node in LDS (parent / depth), then
//                every pair's hop distance from its lowest common ancestor -> a per-tree uint16 table (n_t^2 entries), the
//                tree diameter (its maximum) and the "last node per label" table.
//   pos_pairs    per step, one workgroup of four waves per 64-row block of a tree: the tree's p rows staged in LDS once,
//                lane = row i, wave w sweeps j = w, w + 4, ... with p_j as an LDS broadcast; the four partial sums of a row
//                meet in LDS in a fixed order, then wave 0 writes the full g_p row (pair + compactness terms, the step's
//                weight sum folded in) and the block's two partial sums.  No atomics: each row's gradient needs only its own
//                pairs (A is symmetric, so the two occurrences of a pair give the same term: factor 2).  Four waves per
//                block, not one: a workgroup's LDS (the tree's rows, ~39 KB at 150 nodes) then serves four waves, and a CU
//                keeps enough of them resident to hide the latency of the LDS and table reads.
//   pos_finish   per step, one workgroup per label: the running-mean update of its row of M (absent labels: counter-hash
//                noise), and in workgroup 0 the fixed-order sums of the block partials -> d, c and the loss numerator.
// Every sum has a fixed order: results are run-to-run bitwise reproducible.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include <algorithm>

#include "spgnn_hip.h"
#include "spgnn_internal.h"

using spgnn_detail::check_launch;
using spgnn_detail::fail;

namespace {

constexpr int kTabMaxNodes = 2048;     // LDS-resident parent / depth arrays of the table kernel
constexpr int kMaxLabels = 32;
constexpr int kRows = 64;              // rows per block of the pair kernel = lanes of a wave
constexpr int kMaxCols = 64;
constexpr int kWaves = 4;             // waves of a pair-kernel workgroup: same 64 rows, every kWaves-th j each

__global__ __launch_bounds__(256) void pos_tables(const int32_t* __restrict__ out_indptr, const int32_t* __restrict__ out_indices,
                                                  const int64_t* __restrict__ tree_ptr, const int64_t* __restrict__ dist_off,
                                                  const int64_t* __restrict__ labels, int num_labels, uint16_t* __restrict__ dist,
                                                  int32_t* __restrict__ diameters, int32_t* __restrict__ label_node) {
  __shared__ int depth[kTabMaxNodes], parent[kTabMaxNodes];
  __shared__ int lab[kMaxLabels];
  __shared__ int flag, dmax;
  const int t = blockIdx.x, tid = threadIdx.x;
  const int64_t base = tree_ptr[t];
  const int n = (int)(tree_ptr[t + 1] - base);
  for (int u = tid; u < n; u += 256) { depth[u] = u == 0 ? 0 : -1; parent[u] = -1; }
  if (tid < kMaxLabels) lab[tid] = -1;
  if (tid == 0) dmax = 0;
  // level-synchronous BFS over the tree's edges (both directions are edges of the batched graph; self loops skipped).  In a
  // tree a node of level L + 1 has exactly one neighbour on level L, so the claims below never race.
  for (int L = 0;; ++L) {
    __syncthreads();
    if (tid == 0) flag = 0;
    __syncthreads();
    for (int u = tid; u < n; u += 256) {
      if (depth[u] != L) continue;
      for (int e = out_indptr[base + u]; e < out_indptr[base + u + 1]; ++e) {
        const int v = (int)(out_indices[e] - base);
        if (v < 0 || v >= n || v == u || depth[v] >= 0) continue;
        depth[v] = L + 1;
        parent[v] = u;
        flag = 1;
      }
    }
    __syncthreads();
    if (!flag) break;
  }
  // hop distance of every ordered pair: climb to the lowest common ancestor
  int m = 0;
  uint16_t* __restrict__ tab = dist + dist_off[t];
  for (int64_t idx = tid; idx < (int64_t)n * n; idx += 256) {
    const int i = (int)(idx / n), j = (int)(idx - (int64_t)i * n);
    int a = i, b = j, da = depth[i], db = depth[j];
    if (da < 0 || db < 0) { tab[idx] = 0; continue; }   // not connected to the first node: not a tree (documented as unsupported)
    while (da > db) { a = parent[a]; --da; }
    while (db > da) { b = parent[b]; --db; }
    while (a != b) { a = parent[a]; b = parent[b]; --da; }
    const int h = depth[i] + depth[j] - 2 * da;
    tab[idx] = (uint16_t)h;
    m = max(m, h);
  }
  atomicMax(&dmax, m);                  // max: order-independent
  // the node with the HIGHEST local index per label (the reference's dict comprehension keeps the last one)
  for (int u = tid; u < n; u += 256) {
    const int64_t y = labels[base + u];
    if (y >= 1 && y <= num_labels) atomicMax(&lab[y - 1], u);
  }
  __syncthreads();
  if (tid == 0) diameters[t] = dmax;
  if (tid < num_labels) label_node[(int64_t)t * num_labels + tid] = lab[tid] >= 0 ? (int32_t)(base + lab[tid]) : -1;
}

// uniform [0, 1) noise of an absent label's statistics row: 24 bits of a counter hash of (seed, step, tree, label, column)
__device__ __forceinline__ float pos_noise(uint64_t seed, int64_t step, int64_t t, int L, int k, int num_labels, int D) {
  const uint64_t z = spgnn_detail::mix64(spgnn_detail::mix64(seed, step), (t * num_labels + L) * D + k);
  return (float)(z >> 40) * (1.f / 16777216.f);
}

template <int DP>
__global__ __launch_bounds__(kRows * kWaves) __attribute__((amdgpu_waves_per_eu(1, 3))) void pos_pairs(const float* __restrict__ p, int64_t p_stride, int D, const int64_t* __restrict__ labels,
                                                   const int64_t* __restrict__ tree_ptr, const int64_t* __restrict__ dist_off,
                                                   const uint16_t* __restrict__ dist, const int32_t* __restrict__ diameters,
                                                   const int32_t* __restrict__ label_node, int num_labels, const int32_t* __restrict__ blocks,
                                                   const int32_t* __restrict__ num_trees_dev, const float* __restrict__ mean,
                                                   int64_t* __restrict__ state, const float* __restrict__ weight_sum, float c_weight,
                                                   float* __restrict__ g_p, int64_t g_stride, float* __restrict__ partials) {
  extern __shared__ float lds[];        // n rows of DP floats (columns >= D zero), then T[0 .. diam]; after the sweep: the reduction
  const int blk = blockIdx.x, tid = threadIdx.x, lane = tid & (kRows - 1), wave = tid / kRows;
  const int t = blocks[2 * blk], r0 = blocks[2 * blk + 1];
  const int64_t steps_done = state[0];  // M is set once a step has finished
  __syncthreads();
  if (blk == 0 && tid == 0) state[1] = steps_done;     // pos_finish reads the step index from here (no one else reads it)
  if (t < 0) {                          // unused block of the fixed grid
    if (tid == 0) { partials[2 * blk] = 0.f; partials[2 * blk + 1] = 0.f; }
    return;
  }
  const int64_t base = tree_ptr[t];
  const int n = (int)(tree_ptr[t + 1] - base);
  const int B = *num_trees_dev;
  for (int e = tid; e < n * DP; e += kRows * kWaves) {
    const int r = e / DP, k = e - r * DP;
    lds[e] = k < D ? p[(base + r) * p_stride + k] : 0.f;
  }
  float* __restrict__ T = lds + n * DP;
  const int diam = diameters[t];
  for (int h = tid; h <= diam && h < n; h += kRows * kWaves)             // the reference's float32 all_pos_encs = hops / diam (float64), then exp
    T[h] = diam > 0 ? expf(-(float)((double)h / (double)diam)) : 1.f;
  __syncthreads();
  const int r = r0 + lane;
  const bool act = r < n;
  const int rr = act ? r : n - 1;
  float pi[DP], g[DP];
#pragma unroll
  for (int k = 0; k < DP; k += 4) {
    const float4 v = *reinterpret_cast<const float4*>(lds + rr * DP + k);
    pi[k] = v.x; pi[k + 1] = v.y; pi[k + 2] = v.z; pi[k + 3] = v.w;
    g[k] = g[k + 1] = g[k + 2] = g[k + 3] = 0.f;
  }
  const uint16_t* __restrict__ col = dist + dist_off[t] + rr;   // hops(j, r) = hops(r, j): lanes read consecutive entries
  float lsum = 0.f;
  int hj = wave < n ? col[(int64_t)wave * n] : 0;
  for (int j = wave; j < n; j += kWaves) {
    const float tj = T[hj];
    if (j + kWaves < n) hj = col[(int64_t)(j + kWaves) * n];    // the next table entry is in flight during this pair
    const float* __restrict__ pj = lds + j * DP;
    float d[DP];
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < DP; k += 4) {
      const float4 v = *reinterpret_cast<const float4*>(pj + k);
      d[k] = pi[k] - v.x; d[k + 1] = pi[k + 1] - v.y; d[k + 2] = pi[k + 2] - v.z; d[k + 3] = pi[k + 3] - v.w;
      s += fabsf(d[k]) + fabsf(d[k + 1]) + fabsf(d[k + 2]) + fabsf(d[k + 3]);
    }
    const float a = expf(-s);
    const float diff = a - tj;          // |diff| < 1: smooth-L1 (beta 1) is on its quadratic branch
    lsum = fmaf(0.5f * diff, diff, lsum);
    const float c = -diff * a;
#pragma unroll
    for (int k = 0; k < DP; ++k)        // sign(0) = 0 (torch's abs)
      g[k] += d[k] > 0.f ? c : (d[k] < 0.f ? -c : 0.f);
  }
  // the kWaves partial sums of every row: waves 1 .. kWaves-1 hand theirs to wave 0 in turn (fixed order), through LDS
  __syncthreads();
  float* __restrict__ red = lds;        // 64 rows x (DP + 1) floats, then 64 loss partials
  for (int w = 1; w < kWaves; ++w) {
    if (wave == w) {
#pragma unroll
      for (int k = 0; k < DP; ++k) red[lane * (DP + 1) + k] = g[k];
      red[kRows * (DP + 1) + lane] = lsum;
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
      for (int k = 0; k < DP; ++k) g[k] += red[lane * (DP + 1) + k];
      lsum += red[kRows * (DP + 1) + lane];
    }
    __syncthreads();
  }
  if (wave != 0) return;
  const float wsum = weight_sum ? *weight_sum : 1.f;
  const float scale = wsum * 2.f / ((float)B * (float)n * (float)n);
  float csum = 0.f;
  if (act) {
    const int64_t node = base + r;
    const int64_t y = labels[node];
    const bool comp = steps_done > 0 && y >= 1 && y <= num_labels && label_node[(int64_t)t * num_labels + (y - 1)] == node;
    const float cs = wsum * c_weight * 2.f / (float)B;
    float* __restrict__ out = g_p + node * g_stride;
#pragma unroll
    for (int k = 0; k < DP; ++k) {      // (columns >= D: pi is 0 there, never stored)
      float v = g[k] * scale;
      if (comp && k < D) {
        const float e = pi[k] - mean[(y - 1) * D + k];
        csum = fmaf(e, e, csum);
        v = fmaf(cs, e, v);
      }
      if (k < D) out[k] = v;
    }
  } else {
    lsum = 0.f;
  }
  for (int off = 32; off > 0; off >>= 1) {
    lsum += __shfl_xor(lsum, off, 64);
    csum += __shfl_xor(csum, off, 64);
  }
  if (lane == 0) {
    partials[2 * blk] = lsum / ((float)n * (float)n);
    partials[2 * blk + 1] = csum;
  }
}

__global__ __launch_bounds__(1024) void pos_finish(const float* __restrict__ p, int64_t p_stride, int D, const int32_t* __restrict__ label_node,
                                                   int num_labels, const int32_t* __restrict__ num_trees_dev, const float* __restrict__ partials,
                                                   int num_blocks, float* __restrict__ mean, int64_t* __restrict__ state, uint64_t seed,
                                                   const float* __restrict__ weight_sum, float c_weight, float* __restrict__ loss_num,
                                                   float* __restrict__ losses) {
  __shared__ float red[16][kMaxCols];
  __shared__ float rd[1024], rc[1024];
  const int L = blockIdx.x, tid = threadIdx.x, k = tid & 63, ch = tid >> 6;
  const int B = *num_trees_dev;
  const int64_t step = state[1];
  float acc = 0.f;
  if (k < D) {
    for (int t = ch; t < B; t += 16) {
      const int32_t node = label_node[(int64_t)t * num_labels + L];
      acc += node >= 0 ? p[(int64_t)node * p_stride + k] : pos_noise(seed, step, t, L, k, num_labels, D);
    }
  }
  red[ch][k] = acc;
  if (L == 0) {                          // the step's two losses: fixed-order sums of the pair kernel's block partials
    float a = 0.f, b = 0.f;
    for (int i = tid; i < num_blocks; i += 1024) { a += partials[2 * i]; b += partials[2 * i + 1]; }
    rd[tid] = a; rc[tid] = b;
  }
  __syncthreads();
  if (ch == 0 && k < D) {
    float s = 0.f;
    for (int c = 0; c < 16; ++c) s += red[c][k];
    const float bm = s / (float)B;
    float* m = mean + (int64_t)L * D + k;
    *m = step == 0 ? bm : 0.15f * *m + 0.85f * bm;
  }
  if (L == 0) {
    for (int w = 512; w > 0; w >>= 1) {
      if (tid < w) { rd[tid] += rd[tid + w]; rc[tid] += rc[tid + w]; }
      __syncthreads();
    }
    if (tid == 0) {
      const float d = rd[0] / (float)B, c = rc[0] / (float)B;
      losses[0] = d;
      losses[1] = c;
      if (loss_num) loss_num[0] += (weight_sum ? *weight_sum : 1.f) * (d + c_weight * c);
      state[0] = step + 1;
    }
  }
}

template <int DP>
int launch_pairs(const float* p, int64_t p_stride, int32_t D, const int64_t* labels, const int64_t* tree_ptr, const int64_t* dist_off,
                 const uint16_t* dist, const int32_t* diameters, const int32_t* label_node, int32_t num_labels, const int32_t* blocks,
                 int32_t num_blocks, const int32_t* num_trees_dev, int lds, const float* mean, int64_t* state, const float* weight_sum,
                 float c_weight, float* g_p, int64_t g_stride, float* partials, hipStream_t st) {
  if (lds > 64 * 1024) {
    const int rc = spgnn_detail::ensure_dynamic_lds((const void*)pos_pairs<DP>, lds);
    if (rc != SPGNN_OK) return rc;
  }
  hipLaunchKernelGGL(pos_pairs<DP>, dim3((unsigned)num_blocks), dim3(kRows * kWaves), (size_t)lds, st, p, p_stride, D, labels, tree_ptr, dist_off,
                     dist, diameters, label_node, num_labels, blocks, num_trees_dev, mean, state, weight_sum, c_weight, g_p, g_stride,
                     partials);
  return check_launch("spgnn_pos_losses (pairs)");
}

}  // namespace

extern "C" {

int spgnn_pos_loss_tables(const int32_t* out_indptr, const int32_t* out_indices, const int64_t* tree_ptr, const int64_t* dist_off,
                          const int64_t* labels, int32_t num_labels, int64_t num_trees, int64_t max_tree_nodes, uint16_t* dist,
                          int32_t* diameters, int32_t* label_node, spgnn_stream_t stream) {
  if (num_trees < 0 || max_tree_nodes < 0 || num_labels < 1 || num_labels > kMaxLabels)
    return fail(SPGNN_ERR_SHAPE, "spgnn_pos_loss_tables: bad sizes (1 <= num_labels <= 32)");
  if (num_trees == 0) return SPGNN_OK;
  if (max_tree_nodes > kTabMaxNodes)
    return fail(SPGNN_ERR_SHAPE, "spgnn_pos_loss_tables: a tree exceeds 2048 nodes (LDS-resident parent / depth arrays)");
  if (!out_indptr || !out_indices || !tree_ptr || !dist_off || !labels || !dist || !diameters || !label_node)
    return fail(SPGNN_ERR_NULLPTR, "spgnn_pos_loss_tables: null pointer");
  hipLaunchKernelGGL(pos_tables, dim3((unsigned)num_trees), dim3(256), 0, (hipStream_t)stream, out_indptr, out_indices, tree_ptr,
                     dist_off, labels, num_labels, dist, diameters, label_node);
  return check_launch("spgnn_pos_loss_tables");
}

int spgnn_pos_losses(const float* p, int64_t p_stride, int32_t D, const int64_t* labels, const int64_t* tree_ptr, const int64_t* dist_off,
                     const uint16_t* dist, const int32_t* diameters, const int32_t* label_node, int32_t num_labels, const int32_t* blocks,
                     int32_t num_blocks, const int32_t* num_trees_dev, int64_t max_trees, int64_t max_tree_nodes, float* mean,
                     int64_t* state, uint64_t seed, const float* weight_sum, float c_weight, float* g_p, int64_t g_p_stride,
                     float* partials, float* loss_num, float* losses, spgnn_stream_t stream) {
  if (D < 1 || D > kMaxCols || num_labels < 1 || num_labels > kMaxLabels || num_blocks < 0 || max_trees < 0 || max_tree_nodes < 0)
    return fail(SPGNN_ERR_SHAPE, "spgnn_pos_losses: bad sizes (1 <= D <= 64, 1 <= num_labels <= 32)");
  if (num_blocks == 0 || max_trees == 0) return SPGNN_OK;
  if (!p || !labels || !tree_ptr || !dist_off || !dist || !diameters || !label_node || !blocks || !num_trees_dev || !mean || !state ||
      !g_p || !partials || !losses)
    return fail(SPGNN_ERR_NULLPTR, "spgnn_pos_losses: null pointer");
  if (p_stride < D || g_p_stride < D) return fail(SPGNN_ERR_STRIDE, "spgnn_pos_losses: row stride smaller than row");
  const int DP = D <= 40 ? 40 : 64;     // the two instantiations' row widths in LDS
  const int64_t lds = (int64_t)std::max<int64_t>(max_tree_nodes * (DP + 1), kRows * (DP + 2)) * (int64_t)sizeof(float) + 16;
  if (lds > 160 * 1024) return fail(SPGNN_ERR_SHAPE, "spgnn_pos_losses: a tree's p rows exceed the 160 KiB of LDS");
  const hipStream_t st = (hipStream_t)stream;
  int rc;
  if (DP == 40)
    rc = launch_pairs<40>(p, p_stride, D, labels, tree_ptr, dist_off, dist, diameters, label_node, num_labels, blocks, num_blocks,
                          num_trees_dev, (int)lds, mean, state, weight_sum, c_weight, g_p, g_p_stride, partials, st);
  else
    rc = launch_pairs<64>(p, p_stride, D, labels, tree_ptr, dist_off, dist, diameters, label_node, num_labels, blocks, num_blocks,
                          num_trees_dev, (int)lds, mean, state, weight_sum, c_weight, g_p, g_p_stride, partials, st);
  if (rc != SPGNN_OK) return rc;
  hipLaunchKernelGGL(pos_finish, dim3((unsigned)num_labels), dim3(1024), 0, st, p, p_stride, D, label_node, num_labels, num_trees_dev,
                     partials, num_blocks, mean, state, seed, weight_sum, c_weight, loss_num, losses);
  return check_launch("spgnn_pos_losses (finish)");
}

}  // extern "C"
