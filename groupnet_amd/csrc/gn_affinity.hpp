// Fused cosine affinity + top-k incidence of one scene (A0 + A1: model/GroupNet_nba.py:284-286, model/MS_HGNN_batch.py:372-388)
// as a device function: the stand-alone launch (gn_graph.hip: one workgroup per scene) and the TAIL workgroups of the
// node stage's launch (gn_mlp_bf16.hpp: the first node stage of a forward needs only f, not the incidence, so the two
// are independent; dispatched behind the node stage's own workgroups, the scenes' workgroups fill the CUs its short "A"
// workgroups leave early instead of costing a launch of their own) run the same code.
#pragma once
#include "gn_mlp_common.hpp"

namespace {

struct ScaleList {
  float* H[GN_MAX_SCALES];
  int k[GN_MAX_SCALES];  // clamped to >= 1; k == N marks the single all-ones hyperedge
  int n;
  // optional second destination: the (B, cat_rows, N) concatenation of every H_s (scale s at row cat_off[s])
  float* H_cat;
  int cat_off[GN_MAX_SCALES];
  int cat_rows;
};
// Optional bit-mask form of every H_s (stand-alone launch only: the node stage's tail passes none, so its code is that
// of a launch without masks).  row[s] (B, E_s), col[s] (B, N): bit n of row word (b,e) and bit e of column word (b,n)
// are set iff H_s[b,e,n] != 0.  N <= 64.
struct MaskList {
  unsigned long long* row[GN_MAX_SCALES];
  unsigned long long* col[GN_MAX_SCALES];
};


// Ranking key of affinity v in column j of its row: key_j > key_c  <=>  beats(v_j, j, v_c, c).  High word: the float's
// bits mapped to an order-preserving unsigned (-0 folded into +0: the two compare equal; every NaN -> the largest key:
// NaN ranks first), low word: ~j (the lower index wins a tie).  One 64-bit compare per (j, c) instead of the
// NaN / greater / equal / index cascade — the ranking was the larger half of this kernel at N = 50.
__device__ __forceinline__ unsigned long long rank_key(float v, int j) {
  const float z = v + 0.f;                                   // -0 -> +0
  const uint32_t b = __float_as_uint(z);
  uint32_t s = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  s = (z != z) ? 0xFFFFFFFFu : s;
  return ((unsigned long long)s << 32) | (uint32_t)(~(uint32_t)j);
}
// the writes of every scale for column c of row i, given its rank
template <typename T>
__device__ __forceinline__ void emit_ranked(int rank, int N, int b, int i, int c, const ScaleList& sl) {
  T* H_cat = reinterpret_cast<T*>(sl.H_cat);   // the concatenation is what the caller returns: storage type T
  for (int s = 0; s < sl.n; ++s) {
    if (sl.k[s] == N) {
      if (i == 0) {
        sl.H[s][(size_t)b * N + c] = 1.f;
        if (H_cat) st1(H_cat + ((size_t)b * sl.cat_rows + sl.cat_off[s]) * N + c, 1.f);
      }
    } else {
      const float v = rank < sl.k[s] ? 1.f : 0.f;
      sl.H[s][((size_t)b * N + i) * N + c] = v;
      if (H_cat) st1(H_cat + ((size_t)b * sl.cat_rows + sl.cat_off[s] + i) * N + c, v);
    }
  }
}

// ... of a scene with nb <= N valid agents (gn_affinity_topk_ragged_*, gn_topk_incidence_ragged_f32): `rank` counts the
// columns < nb that beat c, so rank < k selects the top-min(k, nb) of the valid columns; rows and columns >= nb are
// zeros, and the single hyperedge of a scale-N module holds the nb valid agents.
template <typename T>
__device__ __forceinline__ void emit_ranked_ragged(int rank, int nb, int N, int b, int i, int c, const ScaleList& sl) {
  T* H_cat = reinterpret_cast<T*>(sl.H_cat);
  const bool valid = i < nb && c < nb;
  for (int s = 0; s < sl.n; ++s) {
    if (sl.k[s] == N) {
      if (i == 0) {
        const float v = c < nb ? 1.f : 0.f;
        sl.H[s][(size_t)b * N + c] = v;
        if (H_cat) st1(H_cat + ((size_t)b * sl.cat_rows + sl.cat_off[s]) * N + c, v);
      }
    } else {
      const float v = valid && rank < sl.k[s] ? 1.f : 0.f;
      sl.H[s][((size_t)b * N + i) * N + c] = v;
      if (H_cat) st1(H_cat + ((size_t)b * sl.cat_rows + sl.cat_off[s] + i) * N + c, v);
    }
  }
}

// One workgroup per scene.  f rows are normalised into LDS (stride D+4 floats keeps the
// 16-byte row reads of different rows on different banks); corr is formed once per UNORDERED pair (the dot product
// is symmetric term by term, so corr[j][i] is the same bits), optionally written out, and kept in LDS as ranking keys,
// which are then ranked in place.  Needs N*(D+4)*4 + N*N*8 bytes of LDS.
// MASKS (with `ml`): the ranking loop also ORs every member into 2 n_scales N 64-bit words behind the raw inputs (row words
// of scale s at (2s)N, column words at (2s+1)N; zeroed before the first barrier), which one more barrier later go out
// coalesced — read off the same ranks as H_s, order-independent, hence deterministic.
// RAGGED (with `n_valid`, stand-alone launch only): scene b has n_valid[b] (clamped to [0, N]) valid agents, its first
// rows.  Every row is still staged and normalised (padded rows must be finite), the affinity of a pair with a padded end
// is written as 0, the ranking runs over the valid columns alone (emit_ranked_ragged).
template <typename T, bool MASKS = false, bool RAGGED = false>
__device__ __forceinline__ void affinity_topk_body(const T* __restrict__ f, float* __restrict__ corr, const ScaleList& sl,
                                                   int N, int D, const gn_block_extras_t& ex, int b, float* lds,
                                                   const MaskList* ml = nullptr, const int* n_valid = nullptr) {
  constexpr int kBlock = 256;
  int nb = N;
  if constexpr (RAGGED) nb = min(max(n_valid[b], 0), N);
  const int ldq = D + 4;
  float* q = lds;             // N x ldq
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(lds + N * ldq + ((N * ldq) & 1));  // N x N, 8-byte aligned
  const T* fb = f + (size_t)b * N * D;
  const int d4 = D >> 2;
  if (ex.counter != nullptr && b == 0 && threadIdx.x == 0) *ex.counter += ex.counter_add;
  float* xs = reinterpret_cast<float*>(keys + N * N);  // N x x_dim raw inputs (embedding form only)
  unsigned long long* mw = nullptr;                    // 2 x n_scales x N mask words
  if constexpr (MASKS) {
    const int nx = ex.x_raw != nullptr ? N * ex.x_dim : 0;
    mw = reinterpret_cast<unsigned long long*>(xs + nx + (nx & 1));
    for (int idx = threadIdx.x; idx < 2 * sl.n * N; idx += kBlock) mw[idx] = 0ull;
  }
  if (ex.x_raw != nullptr) {
    const float* xb = ex.x_raw + (size_t)b * N * ex.x_dim;
    for (int idx = threadIdx.x; idx < N * ex.x_dim; idx += kBlock) xs[idx] = xb[idx];
    __syncthreads();
  }
  for (int idx = threadIdx.x; idx < N * d4; idx += kBlock) {
    const int r = idx / d4, cc = idx - r * d4;
    f32x4 v;
    if (ex.x_raw != nullptr) {
      // f = M x + c[agent slot]: the whole embedding front-end is one affine map in eval mode
      v = *reinterpret_cast<const f32x4*>(ex.c + (size_t)r * D + 4 * cc);
      const float* xr = xs + r * ex.x_dim;
      for (int k = 0; k < ex.x_dim; ++k) {
        const float xv = xr[k];
        v[0] = fmaf(ex.M[(size_t)(4 * cc + 0) * ex.x_dim + k], xv, v[0]);
        v[1] = fmaf(ex.M[(size_t)(4 * cc + 1) * ex.x_dim + k], xv, v[1]);
        v[2] = fmaf(ex.M[(size_t)(4 * cc + 2) * ex.x_dim + k], xv, v[2]);
        v[3] = fmaf(ex.M[(size_t)(4 * cc + 3) * ex.x_dim + k], xv, v[3]);
      }
      *reinterpret_cast<f32x4*>(ex.f_contig + ((size_t)b * N + r) * D + 4 * cc) = v;
    } else {
      v = ld4(fb + (size_t)r * D + 4 * cc);
    }
    *reinterpret_cast<f32x4*>(q + r * ldq + 4 * cc) = v;
    if (ex.f_out != nullptr) st4(reinterpret_cast<T*>(ex.f_out) + ((size_t)b * N + r) * ex.f_out_ld + 4 * cc, v);
  }
  __syncthreads();
  // row norms: one wave per row, lanes stride the row
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int r = wave; r < N; r += kBlock / 64) {
    float ss = 0.f;
    for (int d = lane; d < D; d += 64) ss += q[r * ldq + d] * q[r * ldq + d];
    ss = gn_wave_sum(ss);
    const float denom = fmaxf(sqrtf(ss), 1e-12f);  // F.normalize eps, GroupNet_nba.py:284
    for (int d = lane; d < D; d += 64) q[r * ldq + d] = q[r * ldq + d] / denom;
  }
  __syncthreads();
  const int Pn = gn_pair_count(N);
  for (int p = threadIdx.x; p < Pn; p += kBlock) {
    int i, j;
    gn_pair_decode(p, N, i, j);
    const f32x4* a = reinterpret_cast<const f32x4*>(q + i * ldq);
    const f32x4* c = reinterpret_cast<const f32x4*>(q + j * ldq);
    float acc = 0.f;
    for (int d = 0; d < d4; ++d) {
      const f32x4 x = a[d], y = c[d];
      acc = fmaf(x[0], y[0], acc);
      acc = fmaf(x[1], y[1], acc);
      acc = fmaf(x[2], y[2], acc);
      acc = fmaf(x[3], y[3], acc);
    }
    if constexpr (RAGGED) {
      if (j >= nb) acc = 0.f;      // (i <= j: a padded end)
    }
    keys[i * N + j] = rank_key(acc, j);
    keys[j * N + i] = rank_key(acc, i);
    if (corr) {
      corr[(size_t)b * N * N + i * N + j] = acc;
      corr[(size_t)b * N * N + j * N + i] = acc;
    }
  }
  if (sl.n == 0) return;
  __syncthreads();
  for (int idx = threadIdx.x; idx < N * N; idx += kBlock) {
    const int i = idx / N, c = idx - i * N;
    const unsigned long long* row = keys + i * N;
    const unsigned long long kc = row[c];
    int rank = 0;
    if constexpr (RAGGED) {
      for (int j = 0; j < nb; ++j) rank += row[j] > kc ? 1 : 0;
      emit_ranked_ragged<T>(rank, nb, N, b, i, c, sl);
    } else {
      for (int j = 0; j < N; ++j) rank += row[j] > kc ? 1 : 0;
      emit_ranked<T>(rank, N, b, i, c, sl);
    }
    if constexpr (MASKS) {
      for (int s = 0; s < sl.n; ++s) {
        if (sl.k[s] != N && rank < sl.k[s]) {
          atomicOr(mw + (2 * s) * N + i, 1ull << c);
          atomicOr(mw + (2 * s + 1) * N + c, 1ull << i);
        }
      }
    }
  }
  if constexpr (MASKS) {
    __syncthreads();
    for (int idx = threadIdx.x; idx < 2 * sl.n * N; idx += kBlock) {
      const int s = idx / (2 * N), r = idx - s * 2 * N;
      const bool all = sl.k[s] == N;          // the single all-ones hyperedge: row word 0 = the N low bits, columns = bit 0
      if (r < N) {
        if (!all) ml->row[s][(size_t)b * N + r] = mw[idx];
        else if (r == 0) ml->row[s][b] = N == 64 ? ~0ull : (1ull << N) - 1ull;
      } else {
        ml->col[s][(size_t)b * N + (r - N)] = all ? 1ull : mw[idx];
      }
    }
  }
}


// host: the scale table of a launch from the caller's lists
inline int fill_scales(ScaleList& sl, float* const* H_list, const int* k_list, int n_scales, int N) {
  sl = ScaleList{};
  if (n_scales < 0 || n_scales > GN_MAX_SCALES) return GN_ERR_SHAPE;
  if (n_scales > 0 && (H_list == nullptr || k_list == nullptr)) return GN_ERR_NULL;
  sl.n = n_scales;
  for (int s = 0; s < n_scales; ++s) {
    if (H_list[s] == nullptr) return GN_ERR_NULL;
    if (k_list[s] > N) return GN_ERR_K_RANGE;
    sl.H[s] = H_list[s];
    sl.k[s] = k_list[s] == N ? N : (k_list[s] < 1 ? 1 : k_list[s]);
    sl.cat_off[s] = sl.cat_rows;
    sl.cat_rows += k_list[s] == N ? 1 : N;
  }
  return GN_OK;
}


// LDS bytes of one scene's workgroup (rows + 64-bit ranking keys (+ raw inputs of the embedding front-end))
inline size_t affinity_fused_lds(int N, int D, int x_dim) {
  return (size_t)N * (D + 4) * sizeof(float) + 8 + (size_t)N * N * 8 + (size_t)N * x_dim * sizeof(float);
}
// ... and of the mask words of a launch that also emits the bit-mask form
inline size_t affinity_mask_lds(int N, int n_scales) { return 8 + (size_t)2 * n_scales * N * 8; }

// host: the fused affinity + top-k job of B scenes — THE statement of its argument checks, in the order every entry that
// issues it answers them, and of the scene tile it needs (`tile`: affinity_fused_lds, plus affinity_mask_lds with mask
// lists), held against `budget`: gn_graph.hip's stand-alone launch allows a workgroup's LDS budget, the node stage's tail
// (gn_mlp_mfma.hip node_plan; no mask lists) its smaller one.  Fills the kernel's scale and mask tables.
// `twin`: bf16 storage.  Pure host code: addresses are tested for NULL and alignment only.
inline int affinity_job_plan(bool twin, const void* f, float* const* H_list, const int* k_list, int n_scales, int B, int N,
                             int D, const gn_block_extras_t* extras, unsigned long long* const* rowmask_list,
                             unsigned long long* const* colmask_list, size_t budget, ScaleList& sl, MaskList& ml,
                             size_t& tile) {
  const bool embed = extras != nullptr && extras->x_raw != nullptr;
  if (embed && twin) return GN_ERR_SHAPE;   // the embedding front-end is fp32 only
  if (!embed) GN_CHECK(need(f, true));
  if (B <= 0 || N <= 0 || D <= 0 || (D & 3) || D > 1024) return GN_ERR_SHAPE;
  GN_CHECK(fill_scales(sl, H_list, k_list, n_scales, N));
  if (embed) {
    if (extras->x_dim <= 0 || !extras->M || !extras->c || !extras->f_contig) return GN_ERR_NULL;
    if (!gn_aligned16(extras->c) || !gn_aligned16(extras->f_contig)) return GN_ERR_ALIGN;
  }
  tile = affinity_fused_lds(N, D, embed ? extras->x_dim : 0);
  ml = MaskList{};
  if (rowmask_list != nullptr || colmask_list != nullptr) {
    if (rowmask_list == nullptr || colmask_list == nullptr) return GN_ERR_NULL;   // both forms or none
    if (N > 64) return GN_ERR_SHAPE;
    for (int s = 0; s < n_scales; ++s) {
      if (rowmask_list[s] == nullptr || colmask_list[s] == nullptr) return GN_ERR_NULL;
      if (!gn_aligned16(rowmask_list[s]) || !gn_aligned16(colmask_list[s])) return GN_ERR_ALIGN;
      ml.row[s] = rowmask_list[s];
      ml.col[s] = colmask_list[s];
    }
    tile += affinity_mask_lds(N, n_scales);
  }
  if (tile > budget) return GN_ERR_LDS;
  if (extras != nullptr) {
    if (extras->f_out != nullptr && (!gn_aligned16(extras->f_out) || extras->f_out_ld < D || (extras->f_out_ld & 3)))
      return GN_ERR_ALIGN;
    sl.H_cat = extras->H_cat;
  }
  return GN_OK;
}

}  // namespace
