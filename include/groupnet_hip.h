/*
 * groupnet_hip.h — C ABI of libgroupnet_hip.so: the MI355X (gfx950) kernels of the
 * GroupNet MS-HGNN hot path.
 *
 * The reference (TaliMotzkin/GroupNet) is pure Python/PyTorch and has no FFI for this
 * path; each entry point below names the reference lines it replaces (paths relative to
 * the reference root).  A host binds them with ctypes/cffi/cgo/JNI: plain pointers and
 * ints only, no torch types.  INTEGRATION.md shows the ctypes stub.
 *
 * Conventions
 *   - every pointer is DEVICE memory owned by the caller, fp32, row-major, contiguous,
 *     16-byte aligned (torch allocations are); inputs are never written;
 *   - `stream` is a hipStream_t (NULL = the default stream); launchers enqueue and return,
 *     they never synchronise, allocate or free — safe to capture in a hipGraph;
 *   - return value: GN_OK (0) or a negative GN_ERR_* code; nothing is launched on error;
 *   - B scenes, N agents (nodes), E hyperedges, K edge types, D = 64 feature width.
 *   - "packed" weights are produced by gn_pack_linear_f32 from an nn.Linear weight
 *     (out x in, row-major); the layout is private to the library.  A kernel that applies several
 *     layers takes ONE buffer holding their packed images back to back, in the order stated.
 *   - bf16 twins (BASELINE config 4: bf16 storage, fp32 accumulate): every stage of the forward
 *     has a *_bf16 entry point taking the SAME descriptor structs.  In a twin the fields marked [T] point to
 *     bf16 tensors (2 bytes per element, 8-byte aligned rows) instead of fp32; incidence H, uniforms U,
 *     edge_feat, biases and the small attention vectors stay fp32; weights are given as the one-part bf16
 *     image (`Wx` fields, gn_split_bf16_f32 with parts = 1).  Products run on v_mfma_f32_32x32x16_bf16 with
 *     fp32 accumulation; a layer's fp32 result is rounded to bf16 (nearest even) when it becomes the next
 *     layer's operand or is stored.  The twins are forward-only (the optional training outputs must be NULL).
 *   - `Wx` images: the fp32-accurate bf16-core path of the *_f32 entry points.  A group that carries `Wx`
 *     (gn_split_bf16_f32 with parts = 3: every weight as three bf16 parts) is evaluated with six bf16
 *     part-products per product on the bf16 matrix cores — as accurate as fp32 accumulation, faster than the
 *     fp32 matrix cores; without it the launch falls back to v_mfma_f32_32x32x2_f32 on the plain packed stream.
 *     Either all groups of a launch carry it or none.
 *   - `Wh` images (`Wh`, `WAh`, `W2h`, `W12h`; ABI 30): the SAME tile stream split into TWO fp16 parts per weight
 *     (gn_split_bf16_f32 with parts = 2) — the "f16x3" path: three v_mfma_f32_32x32x16_f16 part-products per product,
 *     fp32-accurate (3e-7 of max|result| at K = 256), about twice the rate of the six-product bf16 path.  fp16 has a
 *     narrow exponent, so a group that carries `Wh` MUST also carry the corresponding `Wx` image: a workgroup that
 *     meets an operand beyond 65000 in magnitude (or a flagged weight image) repeats its rows on the bf16 path inside
 *     the same launch.  Either all groups of a launch carry `Wh` or none.  The image is followed by a 16-byte FLAG
 *     word that belongs to the split: every split clears it, then raises it when a weight does not fit fp16.
 *   - Order of the tiles in every bf16-/fp16-core image of a LAYER PAIR  out += W1 act(W0 x)  ("pipeline order", the
 *     order the kernels consume them; weights.pipeline_order): with A_t = the first-layer tiles [W0(t, in 0..IT-1)] that
 *     produce hidden tile t and B_t = the second-layer tiles [W1(0..OT-1, t)] that consume it:
 *         A0 A1 B0 A2 B1 ... A(HT-1) B(HT-2) B(HT-1)
 *     (NOT hidden-tile-major [A_t B_t]: A_{t+1} is issued between A_t and B_t so that the splitting of hidden tile t
 *     runs in the shadow of the matrix pipe).  Sub-step offset of A_t: t == 0 ? 0 : NA + (t-1)(NA+NB); of B_t:
 *     t < HT-1 ? 2 NA + t (NA+NB) : HT NA + (HT-1) NB, with NA = 2 IT, NB = 2 OT sub-steps (two per 32x32 tile).
 *   - Node form of the pairwise typed aggregation (gn_agg_group_t.node_form; ABI 33): edge_aggregation.forward reads the
 *     per-edge feature only as H^T feat (MS_HGNN_batch.py:267) and the type weighting and layer 2 are linear, so the
 *     launch can evaluate H^T feat directly, layer 2 once per node instead of once per pair — see the field.  gn_mlp2_*
 *     takes that aggregate with E = 0.
 *   - Closing stage in the aggregation launch (gn_agg_group_t.y ...; ABI 34): the same launch also applies the closing
 *     MLP to cat(H^T feat, ori) / divisor — one launch per message-passing stage fewer, rows bit-identical.
 *   - Bit-mask form of a hyperedge incidence (ABI 37): for N <= 64 (hence E <= 64: E is N or 1) and an H (B,E,N) that holds
 *     only 0 and 1 — every incidence the library builds: top-k, listall, the all-ones edge of scale == N —
 *         rowmask (B,E) 64-bit words: bit n of word (b,e) is set iff H[b,e,n] != 0   (the members of hyperedge e),
 *         colmask (B,N) 64-bit words: bit e of word (b,n) is set iff H[b,e,n] != 0   (the hyperedges of node n).
 *     gn_affinity_topk_* emit it next to H_s, gn_incidence_masks_f32 builds it from any dense H, and the stand-alone gather
 *     and scatter (gn_gather_group_t.rowmask, gn_scatter_group_t.colmask) walk its set bits instead of all N (E) columns
 *     of a dense row.  An H with other weights keeps the dense form.
 *     Also ABI 37, additive (new symbols only: no struct, no signature and no kernel id changed, so the version stays):
 *     gn_node2edge_masks_* hand the row form of the node -> edge pooling the same rowmask words, one 8-byte load per
 *     hyperedge instead of a scan of its dense row.  What still reads the dense H: the banded form of the node -> edge
 *     pooling, gn_node2edge_bwd_*, the pooling inside the edge kernel (N <= 16), and everything at N > 64.
 *   - Ragged batches (ABI 39, additive: new symbols, one new struct and new kernel ids; nothing that existed changed):
 *     scenes of ONE call may hold different numbers of agents.  Tensors keep the padded shapes (B, N, ...); `n_valid` is
 *     a DEVICE array of B ints (4-byte aligned, non-NULL, else GN_ERR_NULL / GN_ERR_ALIGN): scene b's first n_valid[b]
 *     agent rows are real, 1 <= n_valid[b] <= N, the rest is padding.  Every kernel clamps the count it reads to [0, N],
 *     so no address depends on an unchecked value.  Padded input rows must be FINITE (they are read, multiplied by zero
 *     weights, and never reach a valid value); every value at a valid position — node rows n < n_b, pairwise edges (i, j)
 *     with i, j < n_b, hyperedge rows e < n_b or the single row of a scale-N module — is what the same entry point
 *     computes for scene b alone as an n_b-agent scene.  The count enters the arithmetic in four stages, each with an
 *     entry point of its own below (gn_affinity_topk_ragged_*, gn_topk_incidence_ragged_f32, gn_node2edge_ragged_*,
 *     gn_agg_scatter_ragged_*); every other stage is row-wise or reads the padding only through zero entries of H and
 *     needs no count.  gn_zero_padding zeroes the padded positions of the outputs.
 *     The E = 1 shortcut of a module with scale == N is keyed on the padded N: a scene with n_b <= scale < N gets n_b
 *     identical all-member hyperedges (for every scene with n_b > scale the graph is the reference's own).
 *   - Ragged batches from a captured graph (ABI 40, additive: four new symbols and two flag values; no struct, no
 *     signature and no kernel id changed).  A hipGraph captures the ADDRESS of n_valid; the host replaces the values
 *     between replays.  gn_agent_counts_u8 writes them on the device from a (B,N) validity mask, so a mask that already
 *     lives on the GPU costs no read-back.  EMPTY SLOTS: n_valid[b] == 0 is a scene without agents (the unfilled tail of
 *     a static batch).  Every ragged kernel then reads the scene's finite input rows and writes zeros to every output
 *     position of the scene — its incidences and affinities, its edge rows, its node rows — except the single hyperedge
 *     row of a scale-N module, which only goes through row-wise stages: gn_zero_empty_scenes zeroes that one.  No kernel
 *     divides by a count of 0 (the scatter divides only rows n < n_b), and a scene never reads another scene's rows.
 */
#ifndef GROUPNET_HIP_H
#define GROUPNET_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* gn_stream_t; /* hipStream_t */

#define GN_OK 0
#define GN_ERR_NULL -1        /* a required pointer is NULL */
#define GN_ERR_SHAPE -2       /* a size is <= 0 or unsupported (see each function) */
#define GN_ERR_K_RANGE -3     /* top-k: k > N  (torch.topk raises RuntimeError here) */
#define GN_ERR_ALIGN -4       /* a pointer is not 16-byte aligned */
#define GN_ERR_LAUNCH -5      /* hipGetLastError() reported a launch failure */
#define GN_ERR_LDS -6         /* the problem does not fit the 160 KiB LDS tile of the kernel */

#define GN_FEAT 64            /* h_dim == hdim_extend == 64 (MS_HGNN_batch.py:72,292) */
#define GN_MAX_TYPES 16       /* edge types of the typed aggregation, 1 <= K <= 16 (reference: 6 pairwise, 10 hyper): its
                               * per-node first layer and its weight images are laid out per type, up to 16 of them.
                               * The edge head (gn_edge_mlp_gumbel_*) stops at K = 15: logits and factor share ONE 16-row
                               * output tile, rows 0..K-1 the logits and row K the factor pre-activation, so K + 1 <= 16.
                               * A module therefore has 1..15 types; K = 16 exists for the aggregation stage alone.
                               * The node form of the pairwise aggregation (node_form with A) stops at K = 12: the type
                               * weights of a row block, 32 x (16 K + 1) floats, share the LDS with its stage. */
#define GN_MAX_SCALES 8

/* Pitched device-to-device copy of `rows` rows of `width_bytes` (multiples of 16 bytes, 16-byte aligned): the column block of
 * the concatenated feature tensor (model/GroupNet_nba.py:301-309) that a rank ships into its all-gather staging bank. */
int gn_copy_2d(void* dst, size_t dst_pitch, const void* src, size_t src_pitch, size_t width_bytes, int rows,
               gn_stream_t stream);

/* ABI version of this header; bumped on any signature change. */
int gn_abi_version(void);
/* Short static description of a GN_ERR_* code. */
const char* gn_strerror(int code);

/* ---- A0: cosine affinity -------------------------------------------------------------
 * corr[b] = q q^T with q = f / max(||f||_2, 1e-12) per agent.
 * Replaces model/GroupNet_nba.py:284-286 (F.normalize + matmul).
 * f (B,N,D) -> corr (B,N,N).  D must be a multiple of 4, D <= 1024. */
int gn_affinity_f32(const float* f, float* corr, int B, int N, int D, gn_stream_t stream);

/* ---- A1: top-k hyperedge incidence -----------------------------------------------------
 * Replaces MS_HGNN_hyper.init_adj_attention, model/MS_HGNN_batch.py:372-388
 * (torch.topk + zeros().scatter()).  For each of n_scales group sizes k_s:
 *   k_s == N : H_s is (B,1,N), all ones;
 *   else     : k = max(k_s,1); H_s is (B,N,N) with H_s[b,i,c] = 1 iff c is among the k
 *              largest entries of corr[b,i,:]  (ties: lowest index wins; NaN ranks first);
 *   k_s > N  : GN_ERR_K_RANGE.
 * H_list / k_list are HOST arrays of n_scales entries (1 <= n_scales <= GN_MAX_SCALES);
 * one pass over corr serves every scale.  A workgroup stages a band of whole rows of corr in 64 KiB of LDS, so a row
 * must fit there: N <= 16 384, else GN_ERR_LDS (nothing is launched). */
int gn_topk_incidence_f32(const float* corr, float* const* H_list, const int* k_list, int n_scales,
                          int B, int N, gn_stream_t stream);

/* A9: exhaustive hyperedge search — replaces MS_HGNN_hyper.init_adj_attention_listall,
 * model/MS_HGNN_batch.py:390-414 (with its constant candidate table all_combs, :313-326, never
 * materialised): scale == N -> H (B,1,N) all ones; else s = max(scale,1) and H (B,N,N) with row i = the
 * group of s agents containing i that maximises sum_{a,b in group} corr[a][b] over all C(N-1,s-1)
 * candidates (first maximum in the lexicographic candidate order of torch.combinations; NaN ranks first).
 * N <= 64 and C(N-1,s-1) < 2^31, else GN_ERR_SHAPE; scale > N -> GN_ERR_K_RANGE. */
int gn_listall_incidence_f32(const float* corr, float* H, int B, int N, int scale, gn_stream_t stream);

/* A0+A1 fused: f -> corr (may be NULL: not written) and every H_s, without re-reading corr
 * from HBM.  Same contracts as the two functions above; the scene tile, N (D + 4 + x_dim) 4 + 8 + 8 N N bytes (plus
 * 8 + 16 n_scales N with mask lists), must fit 128 KiB of LDS (D = 64: N <= 112; 107 with x_dim = 20), else GN_ERR_LDS:
 * beyond, call gn_affinity_f32 (which switches to its banded kernel there) and gn_topk_incidence_f32.
 * `extras` (may be NULL) lets this first launch of a multiscale forward also produce what the
 * caller's concatenations need, so that no copy kernels follow (model/GroupNet_nba.py:296-311):
 *   f_out   : f is also written to f_out with row stride f_out_ld floats (the first D columns of
 *             the concatenated feature tensor);
 *   H_cat   : every H_s is also written into the (B, sum_s E_s, N) concatenation, scale order;
 *   counter : *counter += counter_add by one thread (advances the device Philox position once per
 *             forward, see gn_edge_mlp_gumbel_f32) — ordered before every later launch of the stream;
 *   x_raw   : the agent embedding itself is computed here: f[b,n] = M x_raw[b,n] + c[n]
 *             with x_raw (B,N,x_dim), M (D,x_dim), c (N,D) — the embedding front-end of
 *             PastEncoder.forward (model/GroupNet_nba.py:269-280), which in eval mode is one affine map
 *             per agent slot; the `f` argument is then ignored and f is ALSO written contiguously to
 *             f_contig (B,N,D), the h_states input of the modules.
 * `rowmask_list` / `colmask_list` (ABI 37; both NULL: not written, else both given): HOST arrays of n_scales device
 * pointers; scale s also receives the bit-mask form of H_s (header comment; the incidence model/MS_HGNN_batch.py:263,267
 * consume) — rowmask_list[s] (B,E_s) and colmask_list[s] (B,N) 64-bit words, 16-byte aligned, read off the same ranks as
 * H_s (the same tie and NaN rules).  k_s == N: rowmask[b,0] = the N low bits, colmask[b,n] = 1.  N <= 64, else
 * GN_ERR_SHAPE.  The tail form of the launch (gn_node_mlp_affinity_*) does not emit masks. */
typedef struct {
  float* f_out;
  int f_out_ld;
  float* H_cat;
  unsigned long long* counter;
  unsigned long long counter_add;
  const float* x_raw;
  int x_dim;
  const float* M;
  const float* c;
  float* f_contig;
} gn_block_extras_t;
int gn_affinity_topk_f32(const float* f, float* corr, float* const* H_list, const int* k_list,
                         int n_scales, int B, int N, int D, const gn_block_extras_t* extras,
                         unsigned long long* const* rowmask_list, unsigned long long* const* colmask_list,
                         gn_stream_t stream);
/* twin: f, extras->f_out and extras->H_cat are bf16 (H values 0/1 are exact in bf16); the normalisation, the
 * affinity and the ranking run in fp32 on the bf16 inputs, corr (may be NULL) and every H_s stay fp32; the
 * embedding front-end (extras->x_raw) is not part of the twin. */
int gn_affinity_topk_bf16(const void* f, float* corr, float* const* H_list, const int* k_list,
                          int n_scales, int B, int N, int D, const gn_block_extras_t* extras,
                          unsigned long long* const* rowmask_list, unsigned long long* const* colmask_list,
                          gn_stream_t stream);

/* The stand-alone fused launch over a ragged batch (header comment; ABI 39).  Row i < n_b of H_s holds the
 * top-min(k_s, n_b) of corr[b, i, :n_b] (the same ranking rules); rows and columns >= n_b of every H_s and of H_cat are
 * zeros; a scale k_s == N is the single hyperedge (B,1,N) holding exactly the n_b valid agents; corr (may be NULL) holds
 * the affinities of the valid block and zeros elsewhere.  extras: f_out, H_cat and counter as above (f_out receives
 * every row of f, padded ones included); the embedding front-end (extras->x_raw) is refused with GN_ERR_SHAPE.  The
 * launch emits no mask lists and is never the node stage's tail. */
int gn_affinity_topk_ragged_f32(const float* f, float* corr, float* const* H_list, const int* k_list, int n_scales,
                                int B, int N, int D, const gn_block_extras_t* extras, const int* n_valid,
                                gn_stream_t stream);
int gn_affinity_topk_ragged_bf16(const void* f, float* corr, float* const* H_list, const int* k_list, int n_scales,
                                 int B, int N, int D, const gn_block_extras_t* extras, const int* n_valid,
                                 gn_stream_t stream);
/* gn_topk_incidence_f32 over a ragged batch, the same rules: corr rows and columns >= n_b are not ranked (they may hold
 * anything finite or not: they are only copied into LDS). */
int gn_topk_incidence_ragged_f32(const float* corr, float* const* H_list, const int* k_list, int n_scales, int B, int N,
                                 const int* n_valid, gn_stream_t stream);

/* Bit-mask form (header comment) of a dense incidence H (B,E,N) — a caller-supplied H, gn_listall_incidence_f32's, the
 * banded top-k's of large N, or one that came out of the node stage's tail: rowmask (B,E), colmask (B,N), the incidence
 * as model/MS_HGNN_batch.py:263,267 consume it.  `nonbinary` (device, may be NULL) receives 1 if any entry is neither 0
 * nor 1 (such an H cannot take this form: keep the dense path), else 0.  E <= 64 and N <= 64, else GN_ERR_SHAPE. */
int gn_incidence_masks_f32(const float* H, int B, int E, int N, unsigned long long* rowmask,
                           unsigned long long* colmask, int* nonbinary, gn_stream_t stream);

/* ---- weight packing -------------------------------------------------------------------
 * Number of floats of the packed image of an (out x in) nn.Linear weight. */
size_t gn_packed_elems(int out_features, int in_features);
/* W (out x in, row-major) -> Wp (gn_packed_elems floats).  The rows/cols are zero-padded to
 * multiples of 32.  `col_offset`/`ld` let a sub-block of a wider matrix be packed:
 * element (o,i) is read from W[o*ld + col_offset + i]. */
int gn_pack_linear_f32(const float* W, float* Wp, int out_features, int in_features, int ld,
                       int col_offset, gn_stream_t stream);

/* Many weights in one launch: segment i drops the source block src (rows x cols, row-major, ld) scaled by
 * `scale` into the packed image starting at dst, at (place_r, place_c) of the image's virtual matrix whose
 * packed rows hold IT 32-column tiles (the layout of gn_pack_linear_f32); IT == 0 writes a plain row-major
 * destination instead: dst[(place_r + r) * dst_ld + place_c + c] = scale * src[r][c] (vectors: rows = 1;
 * concatenated weights for the backward's GEMMs).  Nothing outside the block is written: zero the
 * destination once.
 * `segs` is a DEVICE array (built once per module; the refresh after an optimizer step is then one fill +
 * one launch, capturable in a hipGraph); max_elems = the largest rows*cols of any segment. */
typedef struct {
  const float* src;
  float* dst;
  int ld, rows, cols, place_r, place_c, IT;
  float scale;
  int dst_ld;
} gn_pack_seg_t;
int gn_pack_segments_f32(const gn_pack_seg_t* segs, int n_segs, int max_elems, gn_stream_t stream);

/* ---- grouped launches --------------------------------------------------------------------
 * The 1+S modules of one multiscale forward (pairwise + one hyper module per scale) are
 * independent and differ only in weights, incidence and edge count.  Every stage below
 * therefore takes an array of `n_groups` descriptors (HOST memory, 1 <= n_groups <=
 * GN_MAX_GROUPS) and serves all of them with ONE launch, so that a launch always carries
 * enough workgroups to fill the 256 CUs; a single module is the n_groups == 1 case.
 * Groups must not alias each other's outputs. */
#define GN_MAX_GROUPS 10

/* ---- A3 (first half): node MLP + attention projections -----------------------------------
 * x' = MLP_{64->256->64}(x)            (node2edge_start_mlp, MS_HGNN_batch.py:125,358)
 * pq = x' Wpq^T + bpq  (64 wide)       the node-side halves of attention_mlp layer 0
 *                                      (MS_HGNN_batch.py:131-134,362-365), see gn_node2edge_f32.
 * W    = packed images [W0 (256x64) | W1 (64x256) | Wpq (64x64)] back to back (one weight stream,
 *        consumed in this order); bias = [b0 (256) | b1 (64) | bpq (64)].
 * x (rows,64) -> xp (rows,64), pq (rows,64) per group. */
typedef struct {
  const float* x;   /* [T] */
  const float* W;
  const float* bias;
  float* xp;        /* [T] */
  float* pq;        /* [T] */
  float* hid_out;   /* optional (training): the hidden activations relu(W0 x + b0) (rows, 256) */
  const void* Wx;   /* optional bf16-core image of the chain (72 sub-steps): the layer pair W0 (256x64) / W1 (64x256)
                       in PIPELINE order (header comment: A_t = [W0(t,in0), W0(t,in1)], B_t = [W1(0,t), W1(1,t)],
                       A0 A1 B0 A2 B1 ... A7 B6 B7), then [Wpq(0,in0), Wpq(0,in1), Wpq(1,in0), Wpq(1,in1)].
                       With it W may be NULL. */
  /* optional, with Wx only: the per-node first layer of the typed aggregation MLP of the pairwise graph in the
   * SAME launch (it reads the same node rows; see gn_node_linear_f32): A = WA x + bA, A (rows, KA*128) [T],
   * WAx = bf16-core image of the packed (KA*128 x 64) matrix, bA (KA*128) fp32.  A == NULL: not computed. */
  const void* WAx;
  const float* bA;
  float* A;         /* [T] */
  int KA;
  const void* Wh;   /* optional fp16 two-part image of the same chain stream as Wx (f16x3 path; needs Wx too) */
  const void* WAh;  /* ... of the same stream as WAx (required with Wh when A != NULL) */
} gn_node_group_t;
int gn_node_mlp_f32(const gn_node_group_t* groups, int n_groups, int rows, gn_stream_t stream);
int gn_node_mlp_bf16(const gn_node_group_t* groups, int n_groups, int rows, gn_stream_t stream);
/* The node stage of a forward's FIRST round needs only the agent features, not the incidences: A0 + A1 of the same
 * forward (gn_affinity_topk_*: model/GroupNet_nba.py:284-286, model/MS_HGNN_batch.py:372-388) can ride in the same
 * launch.  `job` = the arguments of gn_affinity_topk_* (f may be NULL with the embedding front-end in `extras`); its B
 * scenes become the launch's TAIL workgroups, dispatched behind the node stage's own and filling the CUs its short
 * workgroups leave early — one launch and one launch boundary fewer (measured at B = 512, N = 11: 7.3 us + 1.3 us).
 * Results are those of the two separate launches, bit for bit.  Needs the groups' bf16-core images (`Wx`) and a scene
 * tile of at most gn_affinity_tail_lds_limit() bytes (N (D + 4 + x_dim) 4 + N N 8 + 8), else GN_ERR_SHAPE / GN_ERR_LDS. */
typedef struct {
  const void* f;             /* [T] (B, N, D) agent features, or NULL with extras->x_raw */
  float* corr;               /* optional (B, N, N) */
  float* const* H_list;      /* n_scales incidence outputs, as gn_affinity_topk_f32 */
  const int* k_list;
  int n_scales;
  int B, N, D;
  const gn_block_extras_t* extras;   /* optional */
} gn_affinity_job_t;
int gn_node_mlp_affinity_f32(const gn_node_group_t* groups, int n_groups, int rows, const gn_affinity_job_t* job,
                             gn_stream_t stream);
int gn_node_mlp_affinity_bf16(const gn_node_group_t* groups, int n_groups, int rows, const gn_affinity_job_t* job,
                              gn_stream_t stream);
size_t gn_affinity_tail_lds_limit(void);
/* Resources of a launch instead of the launch (ABI 35; a host can check the residency it budgets for, the test suite
 * does): what gn_node_mlp_affinity_f32 would pass as dynamic LDS for these arguments (the scene tile of the affinity
 * tail: gn_node_mlp_plan_f32's dyn_lds), and the workgroups per CU the HIP runtime grants the kernel with it (hipOccupancyMaxActiveBlocksPerMultiprocessor).
 * Same argument checks as the launcher; nothing is launched. */
int gn_node_mlp_affinity_launch_info_f32(const gn_node_group_t* groups, int n_groups, int rows, const gn_affinity_job_t* job,
                                         size_t* dyn_lds, int* wgs_per_cu);

/* ---- A3 (second half): attention-weighted node -> edge pooling ---------------------------
 * Replaces the rest of node2edge, MS_HGNN_batch.py:127-141 / 359-370:
 *   e0 = H x';  att[e,n] = w2 . relu(P_n + (H Qn)_e) + b2  with P = pq[:, :32] (bias folded),
 *   Qn = pq[:, 32:];  W = softmax_n(att * H) * H;  edges = W x'.
 * H == NULL selects the pairwise graph of MS_HGNN_oridinary (E must be N*N; edge e = i*N + j has
 * weight 1 on i and on j, 2 when i == j; MS_HGNN_batch.py:118,124,143-160) without ever
 * materialising it.  xp, pq (B,N,64); H (B,E,N) or NULL; w2 (32 floats, device); edges (B,E,64).
 * Symmetric pairwise form (H == NULL, sym = 1): edge (i,j) and edge (j,i) of the pairwise graph carry
 * the same pooled feature, so only the N(N+1)/2 unordered pairs are produced: E = N(N+1)/2, row
 * p(i,j) = i*N - i(i-1)/2 + (j-i) for i <= j.  Every pairwise stage below has the matching form. */
typedef struct {
  const float* xp;   /* [T] */
  const float* pq;   /* [T] */
  const float* H;
  const float* w2;
  float* edges;      /* [T] */
  const float* b2;   /* device pointer to the scalar bias of attention layer 1 (the parameter itself: no
                        host read-back, so a training step stays capturable in a hipGraph) */
  int E;
  int sym;
} gn_n2e_group_t;
int gn_node2edge_f32(const gn_n2e_group_t* groups, int n_groups, int B, int N, gn_stream_t stream);
int gn_node2edge_bf16(const gn_n2e_group_t* groups, int n_groups, int B, int N, gn_stream_t stream);
/* The same launch with the bit-mask form of the hyper groups' incidences (ABI 37, additive; header comment).  `rowmasks`
 * is a HOST array of n_groups device pointers: rowmasks[g] = the (B,E_g) member words of group g, or NULL.  A hyper group
 * still carries its non-NULL H (H == NULL keeps meaning "pairwise", and the banded form reads H); its H must hold only
 * 0 and 1, then the rows are bit-identical to gn_node2edge_*'s.  Where the launch takes the row form (plan variant 1
 * without words) it reads the words instead of H (variant 2); where it takes the banded form the words are ignored.
 * Checked before anything is launched: rowmasks == NULL: GN_ERR_NULL; a word pointer on a pairwise group, any word
 * pointer with N > 64, or words on some hyper groups only (one form per launch): GN_ERR_SHAPE; a word pointer that is not
 * 8-byte aligned: GN_ERR_ALIGN.  All entries NULL: exactly gn_node2edge_* (which are this case of the same code). */
int gn_node2edge_masks_f32(const gn_n2e_group_t* groups, const unsigned long long* const* rowmasks, int n_groups, int B,
                           int N, gn_stream_t stream);
int gn_node2edge_masks_bf16(const gn_n2e_group_t* groups, const unsigned long long* const* rowmasks, int n_groups, int B,
                            int N, gn_stream_t stream);

/* The same launch over a ragged batch (header comment; ABI 39): softmax(att * H) * H runs over the scene's n_b nodes —
 * the non-member term is (n_b - members) exp(0 - max), and the 0 enters the running max only if such a non-member
 * exists.  Hyper groups: dense H (banded or row form as gn_node2edge_* choose), whose columns >= n_b must be zeros (the
 * ragged incidence launches write them so); rows of all-zero hyperedges come out as zeros.  Pairwise groups (ordered or
 * sym): only pairs with both ends < n_b exist; every other edge row is written as zeros. */
int gn_node2edge_ragged_f32(const gn_n2e_group_t* groups, int n_groups, int B, int N, const int* n_valid,
                            gn_stream_t stream);
int gn_node2edge_ragged_bf16(const gn_n2e_group_t* groups, int n_groups, int B, int N, const int* n_valid,
                             gn_stream_t stream);

/* ---- A4: per-edge MLPs + Gumbel-softmax edge typing ----------------------------------------
 * Replaces MLP_dict_softmax.forward + gumbel_softmax, MS_HGNN_batch.py:41-53,446-520:
 *   z = MLP_{64->128->64}(edges); logits = MLP_{64->128->K}(z); fac = sigmoid(MLP_{64->128->1}(z));
 *   g = -log(1e-10 - log(U + 1e-10)); dist = softmax((logits + g) / tau); edge_feat = fac * dist.
 * W = the packed images of Wi0 = init_MLP.0 (128x64), Wi1 = init_MLP.1 (64x128), Wd0 (256x64) and
 *   Wd1 (32x256), where Wd0 = [MLP_distribution.layers.0 ; MLP_factor.layers.0] and Wd1 is the block
 *   matrix whose rows 0..K-1 are [MLP_distribution.layers.1, 0] and row K is [0, MLP_factor.layers.1],
 *   cut into hidden tiles T (8 steps of 256 floats) and second-layer slices S and ordered as the kernel
 *   consumes them:  Wi0/Wi1: T0 T1 S0 T2 S1 T3 S2 S3 (S_t = Wi1 tiles (0,t),(1,t): 8 steps);
 *   Wd0/Wd1: T0 T1 S0 T2 S1 ... T7 S6 S7 (S_t = Wd1 tile (0,t): 4 steps); then 8 steps of padding;
 * bias = [128 | 64 | 256 | 32] in the same order (bd1: K logits biases, then the factor bias, zeros).
 * edges (rows,64), U (rows,K) uniforms in [0,1) -> edge_feat (rows,K), dist (rows,K).  1 <= K <= 15 (row K of the
 *   16-row tile of Wd1 is the factor head: see GN_MAX_TYPES); anything else is GN_ERR_SHAPE.
 * U == NULL: the uniforms are generated inside the kernel — element row*K + k is element
 * philox_offset (+ *offset_dev if not NULL) + row*K + k of the Philox stream `seed`, exactly what
 * gn_philox_uniform_f32 would have written into U.
 * Symmetric pairwise form (sym_N = N > 0): rows = B*N(N+1)/2 unordered pairs.  The MLPs run once per
 * pair; the Gumbel softmax runs for BOTH ordered edges (i,j) and (j,i) with their own uniforms
 * (U / Philox positions are those of the ordered (B,N*N,K) tensor).  dist (B*N*N,K) receives the ordered
 * distributions (may be NULL when the caller does not need them); edge_feat (rows,K) receives
 * fac*(dist_ij + dist_ji) (2*fac*dist_ii on the diagonal) — exactly the weight the pair carries in the
 * edge->node sum, where both ordered edges meet the same typed MLP output. */
typedef struct {
  const float* edges;   /* [T] */
  const float* U;
  const float* W;
  const float* bias;
  float* edge_feat;
  float* dist;          /* [T] */
  unsigned long long philox_offset;
  int rows;
  int K;
  int sym_N;
  /* optional (training), all (rows, .): hidden of init_MLP (128), z (64), hidden of MLP_distribution |
   * MLP_factor (256), and the 32-wide (logits | factor pre-activation | 0) tile — what the backward needs and
   * the kernel otherwise keeps in registers */
  float* keep_z1;
  float* keep_z;
  float* keep_dh1;
  float* keep_lgf;
  const void* Wx;    /* optional bf16-core image (gn_split_bf16_f32) of the fp32 tile stream of the four layers, two
                        layer pairs in PIPELINE order (header comment) — pair A (init_MLP, 4 hidden tiles): A_t =
                        [Wi0(t,in0), Wi0(t,in1)], B_t = [Wi1(0,t), Wi1(1,t)]; pair B (8 hidden tiles): A_t =
                        [Wd0(t,in0), Wd0(t,in1)], B_t = [Wd1(0,t)] — 40 tiles = 80 sub-steps.  With it W may be NULL. */
  /* Fused node->edge pooling (bf16-core kernels only, i.e. with Wx): edges == NULL and xp != NULL — every row of
   * `edges` is formed inside the kernel exactly as gn_node2edge_* would have written it (MS_HGNN_batch.py:127-141,
   * 359-370) and never touches HBM.  xp / pq: (B*N, 64) outputs of gn_node_mlp_*; w2 (32), b2 (1): attention layer 1;
   * pool_N = N; pool_H == NULL: the implicit pairwise graph (unordered pairs when sym_N = N, else the N*N ordered
   * edges); pool_H != NULL: (rows, N) incidence of a hyper module with pool_E hyperedges per scene, N <= 16. */
  const float* xp;      /* [T] */
  const float* pq;      /* [T] */
  const float* pool_H;
  const float* w2;
  const float* b2;
  int pool_N;
  int pool_E;
  const void* Wh;    /* optional fp16 two-part image of the same stream as Wx (f16x3 path; needs Wx too) */
} gn_edge_group_t;
int gn_edge_mlp_gumbel_f32(const gn_edge_group_t* groups, int n_groups, float tau, unsigned long long seed,
                           const unsigned long long* offset_dev, gn_stream_t stream);
int gn_edge_mlp_gumbel_bf16(const gn_edge_group_t* groups, int n_groups, float tau, unsigned long long seed,
                            const unsigned long long* offset_dev, gn_stream_t stream);
/* Resources of gn_edge_mlp_gumbel_f32's launch for groups with the `Wx` image (ABI 35; as
 * gn_node_mlp_affinity_launch_info_f32): dynamic LDS = the kernel's weight ring and the pool stage of the fused pooling,
 * which share one region (GN_POOL_STAGE is honoured). */
int gn_edge_mlp_gumbel_launch_info_f32(const gn_edge_group_t* groups, int n_groups, size_t* dyn_lds, int* wgs_per_cu);

/* ---- A5: hyperedge aggregation --------------------------------------------------------------
 * gather: eo = H ori            (edge_aggregation.forward, MS_HGNN_batch.py:263)
 * H == NULL: pairwise graph (E = N*N), eo[(i,j)] = ori_i + ori_j; with sym = 1 only the
 * E = N(N+1)/2 unordered pairs.   ori (B,N,64) -> eo (B,E,64). */
typedef struct {
  const float* ori;   /* [T] */
  const float* H;
  float* eo;          /* [T] */
  int E;
  int sym;
  const unsigned long long* rowmask;   /* optional (ABI 37): the bit-mask form of H, (B,E) words (model/MS_HGNN_batch.py:263:
                                          eo[b,e] = the sum of ori[b,n] over the set bits n, ascending).  With it H is not
                                          read (may be NULL), sym must be 0 and N <= 64 (else GN_ERR_SHAPE); all hyper
                                          groups of a launch use one form (else GN_ERR_SHAPE).  Rows equal the dense
                                          form's bit for bit on finite ori; the dense form lets a non-finite value of a
                                          NON-member row leak (0 * inf), the mask form does not. */
} gn_gather_group_t;
int gn_agg_gather_f32(const gn_gather_group_t* groups, int n_groups, int B, int N, gn_stream_t stream);
int gn_agg_gather_bf16(const gn_gather_group_t* groups, int n_groups, int B, int N, gn_stream_t stream);

/* typed MLP: feat = sum_k edge_feat[:,k] * MLP^k_{64->128->64}(eo)   (MS_HGNN_batch.py:262,264-265)
 * W: for each type k the packed images [agg_mlp[k].layers.0 (128x64) | agg_mlp[k].layers.1 (64x128)],
 * types back to back; b1 (K,128); b2 (K,64).  eo (rows,64), edge_feat (rows,K) -> feat (rows,64).
 * Fused gather (eo == NULL): the kernel forms its input rows itself from ori (B,N,64) exactly as
 * gn_agg_gather_f32 would — row r = b*E + e is sum_n H[b,e,n] ori[b,n] (H (B,E,N)), or for the
 * pairwise graph (H == NULL) ori_i + ori_j with (i,j) the ordered edge (E = N*N) or the unordered
 * pair (sym = 1, E = N(N+1)/2) — so eo never exists in HBM.  rows must equal B*E.
 * Pair form (A != NULL; pairwise graph, symmetric rows, E = N(N+1)/2): A (B*N, K*128) holds the
 * per-node first layer W1k ori + b1k/2 (gn_node_linear_f32); row p = (i <= j) computes
 * sum_k edge_feat[p,k] * (W2k relu(A[i,k] + A[j,k]) + b2k).  W then is, per type, the packed (64 x 128)
 * image re-ordered hidden-tile-major ((t, o) instead of (o, t)); b1 is unused. */
typedef struct {
  const float* eo;     /* [T] */
  const float* edge_feat;
  const float* W;
  const float* b1;
  const float* b2;
  float* feat;         /* [T] */
  int rows;
  int K;
  const float* ori;    /* [T] */
  const float* H;
  int E;
  int N;
  int sym;
  const float* A;
  const void* W2x;    /* optional, pair form (fp32 entry point only): bf16-core image of layer 2 of every type
                         (gn_split_bf16_f32 of the hidden-tile-major W image: per type and hidden tile t the tiles
                         [W2k(0,t), W2k(1,t)], 16 sub-steps per type) */
  const void* W12x;   /* optional, two-layer form: bf16-core image of both layers, per type one layer pair in PIPELINE
                         order (header comment): A_t = [W1k(t, in 0), W1k(t, in 1)], B_t = [W2k(out 0, t), W2k(out 1, t)],
                         A0 A1 B0 A2 B1 A3 B2 B3 (32 sub-steps per type).  With W2x / W12x, W may be NULL. */
  const void* W2h;    /* optional fp16 two-part images of the same streams as W2x / W12x (f16x3 path; need those too) */
  const void* W12h;
  int node_form;      /* pair form with W2x, N <= 16, K <= 12 only.  Nothing downstream of edge_aggregation.forward reads the
                         per-edge feature: MS_HGNN_batch.py:267 consumes it as H^T feat, and both the type weighting and
                         layer 2 are linear, so they commute with that sum.  With node_form = 1 the kernel evaluates
                           S[n,k] = sum_j edge_feat[p(n,j),k] relu(A[n,k] + A[j,k]),  c[n,k] = sum_j edge_feat[p(n,j),k]
                           (H^T feat)[n] = sum_k (W2k S[n,k] + b2k c[n,k])
                         i.e. layer 2 once per NODE (B*N rows) instead of once per pair (B*N(N+1)/2 rows), and `feat`
                         receives (H^T feat) (B*N, 64) — what gn_mlp2_f32 takes with E = 0.  rows stays B*E. */
  /* Fused closing stage (ABI 34; fp32 entry point on the fp16/bf16-core images, N <= 16; for EVERY group of a launch or
   * for none): with y != NULL the workgroups that finish a scene's aggregate also apply the closing MLP
   *   y[b*N + n] = W1 relu(W0 cat(H^T feat, ori)[n] / divisor + b0) + b1     (MS_HGNN_batch.py:267, :120 / :355, :220-229)
   * — what gn_mlp2_f32 would have computed from `feat` in a launch of its own — and `feat` is neither written nor
   * read (may be NULL).  m2x / m2h / m2bias: gn_mlp2_group_t.Wx / Wh / bias of a 128 -> 128 -> dout MLP, 32 < dout <= 64; y rows
   * have stride ldy.  Needs ori and, for a hyper group, H / E / N with the fused gather (eo == NULL, E <= 16); a
   * pairwise group must use node_form.  Groups too large for the per-scene workgroup shapes (more than 767 row blocks
   * of edge rows) are refused: use the two launches. */
  const void* m2x;
  const void* m2h;
  const float* m2bias;
  float* y;
  int ldy;
  int dout;
  float divisor;
} gn_agg_group_t;
int gn_agg_mlp_f32(const gn_agg_group_t* groups, int n_groups, gn_stream_t stream);
/* twin: two-layer form only (eo, or the fused gather from ori) — a per-node first layer stored in bf16 would
 * cost as much VALU / LDS work per pair as the layer itself costs on the bf16 cores */
int gn_agg_mlp_bf16(const gn_agg_group_t* groups, int n_groups, gn_stream_t stream);
/* Packed fp32 32x32 weight tiles (gn_pack_linear_f32 layout, n_tiles of 1024 floats) -> bf16-core image: for
 * every tile and each of its two k-halves (one "sub-step") `parts` bf16 parts in the A-operand order of
 * v_mfma_f32_32x32x16_bf16: out[(((tile*2 + half)*parts + part)*64 + lane)*8 + j] (16-bit words), where
 * element j of lane (m, h) is the weight of output m and k-feature 16*half + (j&3) + 8*(j>>2) + 4*h — the
 * order in which a lane's accumulator registers hold those features.  parts = 3: x = p1 + p2 + p3 (8 mantissa
 * bits each, round to nearest: the fp32-accurate path); parts = 1: p1 = x rounded to bf16 (the bf16 twins);
 * parts = 2: TWO fp16 parts x = hi + lo (the `Wh` images of the f16x3 path) — `out` then holds 16 more bytes behind
 * the image, the FLAG word, which every split clears (a one-thread launch ahead of it on `stream`) and then raises
 * when a weight is not |x| <= 65000 (NaN included): the flag follows the weights of the LAST split. */
int gn_split_bf16_f32(const float* packed, void* out, int n_tiles, int parts, gn_stream_t stream);
/* The same for `n_jobs` images in ONE launch (job table in DEVICE memory; max_tiles = the largest n_tiles): what a
 * training step needs after its optimizer update — every weight image of every module, one launch after the one
 * gn_pack_segments_f32 launch over the concatenated segment tables — instead of one launch per image (38 launches
 * of ~4 us each per step of the multiscale block; the reference re-reads its nn.Parameters directly,
 * train_hyper_nba.py:107-118). */
typedef struct {
  const float* packed;
  void* out;
  int n_tiles;
  int reserved;
} gn_split_job_t;
int gn_split_bf16_batch_f32(const gn_split_job_t* jobs, int n_jobs, int max_tiles, int parts, gn_stream_t stream);

/* ---- A5, pairwise graph, layer 1 hoisted to the nodes -----------------------------------------
 * For the pairwise graph the typed MLP's input row is eo = ori_i + ori_j, so its first layer is
 * linear in the two nodes: W1k eo + b1k = (W1k ori_i + b1k/2) + (W1k ori_j + b1k/2).  The first layer
 * therefore runs once per NODE (N rows per scene instead of N(N+1)/2 pairs):
 *   y = W x + bias, x (rows,64) -> y (rows,dout), dout a multiple of 128 (W = packed (dout x 64)
 *   image; used with W = [W1_0; ...; W1_{K-1}], bias = b1/2 to produce A (B*N, K*128)); the pair form
 *   of gn_agg_mlp_f32 (field A) then applies relu and the second layer per unordered pair. */
int gn_node_linear_f32(const float* x, const float* W, const float* bias, float* y, int rows, int dout,
                       gn_stream_t stream);

/* scatter: out = cat(H^T feat, ori) / divisor     (MS_HGNN_batch.py:267; divisor = N gives the
 * division of edge2node :120,355, divisor = 1 the bare edge_aggregation.forward).
 * feat (B,E,64), ori (B,N,64) -> out (B,N,128).  H == NULL: pairwise (E = N*N); with sym = 1 feat
 * holds the E = N(N+1)/2 pair sums (see gn_edge_mlp_gumbel_f32) and node n adds the N pairs {n,j}. */
typedef struct {
  const float* feat;   /* [T] */
  const float* H;
  const float* ori;    /* [T] */
  float* out;          /* [T] */
  int E;
  int sym;
  const unsigned long long* colmask;   /* optional (ABI 37): the bit-mask form of H, (B,N) words (model/MS_HGNN_batch.py:267:
                                          node n adds feat[b,e] over the set bits e, ascending).  With it H is not read
                                          (may be NULL), sym must be 0, N <= 64 and E <= 64 (else GN_ERR_SHAPE); all hyper
                                          groups of a launch use one form.  Bit-identical to the dense form. */
} gn_scatter_group_t;
int gn_agg_scatter_f32(const gn_scatter_group_t* groups, int n_groups, int B, int N, float divisor,
                       gn_stream_t stream);
int gn_agg_scatter_bf16(const gn_scatter_group_t* groups, int n_groups, int B, int N, float divisor,
                        gn_stream_t stream);

/* The scatter over a ragged batch (header comment; ABI 39), every group in ONE launch of one straightforward kernel:
 * node n < n_b receives cat(H^T feat, ori)[n] / divisor — a hyper group (dense H; colmask must be NULL) adds its
 * hyperedges, a pairwise group (ordered, or sym) its partners j < n_b only.  divisor == 0 divides each scene by its own
 * n_b (edge2node); a positive divisor behaves as in gn_agg_scatter_*.  Rows n >= n_b of out are written as zeros. */
int gn_agg_scatter_ragged_f32(const gn_scatter_group_t* groups, int n_groups, int B, int N, float divisor,
                              const int* n_valid, gn_stream_t stream);
int gn_agg_scatter_ragged_bf16(const gn_scatter_group_t* groups, int n_groups, int B, int N, float divisor,
                               const int* n_valid, gn_stream_t stream);

/* Zeroes the padded positions of up to GN_MAX_ZERO_ITEMS tensors of a ragged batch in ONE launch (ABI 39): what a ragged
 * forward ends with, whatever its number of modules.  `items` is a HOST array.  A tensor is `rows per scene` rows of
 * `width` bytes at a pitch of `pitch` bytes (a column block of a wider tensor has pitch > width); width, pitch and the
 * address are multiples of 2, else GN_ERR_ALIGN (rows are written as 4-byte words where all three are multiples of 4,
 * else as 2-byte words: a bf16 row of an odd number of elements).  kind: GN_ZERO_NODE_ROWS — (B,N,.), rows n >= n_b; GN_ZERO_EDGE_ROWS —
 * the (B,N,.) hyperedge rows of a top-k module, rows e >= n_b (the single row of a scale-N module is always valid: do
 * not list it); GN_ZERO_PAIR_ROWS — (B,N*N,.) ordered pair rows i*N + j with i >= n_b or j >= n_b (also an (B,N,N)
 * matrix with width = the element size: corr, H, new_H); GN_ZERO_SYM_PAIR_ROWS (an addition within ABI 40: the
 * ragged backward's dfeat) — (B,N(N+1)/2,.) unordered pair rows (i, j >= i), row-major, with j >= n_b (an end of the pair
 * is padding).  Valid positions are not touched.  Any other kind — 3 among them, which ABI 39 and 40 refused and callers
 * may rely on — is GN_ERR_SHAPE. */
#define GN_MAX_ZERO_ITEMS 24
#define GN_ZERO_NODE_ROWS 0
#define GN_ZERO_EDGE_ROWS 1
#define GN_ZERO_PAIR_ROWS 2
#define GN_ZERO_SYM_PAIR_ROWS 4
typedef struct {
  void* ptr;
  long long pitch;
  int width;
  int kind;
} gn_zero_item_t;
int gn_zero_padding(const gn_zero_item_t* items, int n_items, int B, int N, const int* n_valid, gn_stream_t stream);

/* Zeroes whole scenes of up to GN_MAX_ZERO_ITEMS tensors where the scene is an empty slot, n_valid[b] <= 0 (ABI 40): the
 * single hyperedge row (B,1,.) of a scale-N module, which gn_zero_padding does not take.  `items` is a HOST array; here
 * `pitch` is the distance between SCENES in bytes and `width` the bytes of a scene that are zeroed (the same alignment
 * rules and error codes as gn_zero_padding); `kind` is not read.  Scenes with a count >= 1 are not touched. */
int gn_zero_empty_scenes(const gn_zero_item_t* items, int n_items, int B, const int* n_valid, gn_stream_t stream);

/* Agent counts from a validity mask (ABI 40).  valid: (B,N) bytes on the device, any alignment; n_valid[b] = the length
 * of the LEADING RUN of non-zero bytes of valid[b,:] (B ints; 4-byte aligned).  `status` is one device word (4-byte
 * aligned) that the kernel only ever ORs into — sticky: the caller zeroes it once and reads it when it likes:
 * GN_COUNTS_NOT_PREFIX — some scene has a non-zero byte behind a zero byte (those agents are NOT counted: the library
 * has no non-prefix form); GN_COUNTS_EMPTY — some scene has count 0 (legal: an empty slot; informational).
 * One wave per scene, rows beyond 64 agents in chunks of a wave; any N >= 1 and B >= 1, else GN_ERR_SHAPE; a NULL
 * pointer: GN_ERR_NULL; a misaligned n_valid or status: GN_ERR_ALIGN. */
#define GN_COUNTS_NOT_PREFIX 1u
#define GN_COUNTS_EMPTY 2u
int gn_agent_counts_u8(const unsigned char* valid, int B, int N, int* n_valid, unsigned int* status, gn_stream_t stream);

/* The subset of a validity mask WITH HOLES (an addition within ABI 40).  valid: (B,N) bytes on the device, any alignment,
 * non-zero = valid.  With V_b the valid slots of scene b in increasing order and n_b = |V_b|:
 *   n_valid[b]  = n_b                                                    (B ints)
 *   order[b,r]  = the slot of the r-th valid agent for r < n_b, else -1  (B*N ints)
 *   slot[b,n]   = the rank of slot n within V_b, -1 where n is invalid   (B*N ints)
 * The compaction is stable: valid agents keep their relative order.  `status` is the sticky word of gn_agent_counts_u8;
 * this entry point ORs in GN_COUNTS_EMPTY only (a scene without a valid agent) and never GN_COUNTS_NOT_PREFIX.  One wave
 * per scene, rows beyond 64 agents in chunks of a wave with the running base carried from chunk to chunk; any N >= 1 and
 * B >= 1, else GN_ERR_SHAPE; a NULL pointer: GN_ERR_NULL; a misaligned n_valid, order, slot or status (4 bytes):
 * GN_ERR_ALIGN. */
int gn_agent_subset_u8(const unsigned char* valid, int B, int N, int* n_valid, int* order, int* slot, unsigned int* status,
                       gn_stream_t stream);

/* Moves the rows of up to GN_MAX_ZERO_ITEMS tensors through a per-scene index map in ONE launch (an addition within ABI
 * 40): for every destination row, dst[row] = map[...] >= 0 ? src[mapped row] : 0.  map: (B,N) ints on the device, entries
 * in -1 .. N - 1 (anything else counts as -1).  With map = order of gn_agent_subset_u8 this is the COMPACTION of a batch
 * whose scenes have agents missing anywhere (valid rows first, in order, zeros behind them); with map = slot it is the
 * EXPANSION of results back to the original slots (zeros at invalid positions).  `items` is a HOST array; every field
 * is in bytes.  kind: GN_REMAP_NODE_ROWS — N rows per scene, row r of scene b from source row map[b,r];
 * GN_REMAP_PAIR_ROWS — N*N ordered pair rows, row i*N + j from source row map[b,i]*N + map[b,j], zero when either is -1.
 * A (B,N,N) matrix is the pair kind with width = the element size (corr, a top-k H, a scale block of new_H through its
 * own scene stride); the (B,1,N) row of a scale-N module's H is the node kind on its (B,N,1) view.  Every destination
 * position is written exactly once (no scatter, no atomics).  Store unit per item: the largest of 16 / 8 / 4 / 2 bytes
 * that divides both addresses, both scene strides, both pitches and the width (256-byte fp32 feature rows: 16; 24-byte
 * fp32 factor rows: 8; an 18-byte bf16 row: 2); an odd value among them: GN_ERR_ALIGN.  Source and destination of an item
 * MUST NOT OVERLAP (rows are read after other rows were written).  N <= 32767. */
#define GN_REMAP_NODE_ROWS 0
#define GN_REMAP_PAIR_ROWS 1
typedef struct {
  const void* src;
  void* dst;
  long long src_scene;   /* bytes from a scene to the next */
  long long dst_scene;
  long long src_pitch;   /* bytes from a row to the next */
  long long dst_pitch;
  int width;             /* bytes of a row that are moved */
  int kind;              /* GN_REMAP_* */
} gn_remap_item_t;
int gn_remap_rows(const gn_remap_item_t* items, int n_items, int B, int N, const int* map, gn_stream_t stream);

/* ---- A6 / generic two-layer MLP ---------------------------------------------------------------
 * y = W1 relu(W0 x + b0) + b1     (MLP.forward with one hidden layer, MS_HGNN_batch.py:220-229;
 * nmp_mlp_end 128->128->bottleneck and nmp_mlps[even] 128->128->64).
 * din in {64,128}, dh in {128,256}, dout >= 1 (the same for every group).
 * W = packed [W0 (dh x din) | W1 (dout x dh)]; bias = [b0 (dh) | b1 zero-padded to a multiple of 32].
 * x (rows,din) -> y (rows,dout) with row stride ldy >= dout floats (lets the result land in a
 * column block of a wider tensor, e.g. the concatenated per-scale features).
 * Fused scatter (x == NULL, din == 128): the kernel forms its input rows itself exactly as
 * gn_agg_scatter_f32 would — row b*N + n is cat(sum_e H[b,e,n] feat[b,e], ori[b,n]) / divisor
 * (H (B,E,N); H == NULL: the pairwise graph, E = N*N ordered edges or, sym = 1, E = N(N+1)/2 pair
 * sums) — so the (B,N,128) aggregate never exists in HBM.  rows must equal B*N.
 * E == 0 (x == NULL): `feat` already holds H^T feat per node, (rows, 64) — the output of gn_agg_mlp_f32's node form;
 * the input row is cat(feat[row], ori[row]) / divisor. */
typedef struct {
  const float* x;      /* [T] */
  const float* W;
  const float* bias;
  float* y;            /* [T] */
  const float* feat;   /* [T] */
  const float* H;
  const float* ori;    /* [T] */
  int E;
  int sym;
  float* in_out;    /* optional (training): the MLP's input rows as evaluated (rows, din) — with the fused
                       scatter that is cat(H^T feat, ori)/N, which otherwise never exists in memory */
  float* hid_out;   /* optional (training): the hidden activations relu(W0 x + b0) (rows, dh) */
  const void* Wx;   /* optional bf16-core image, one layer pair in PIPELINE order (header comment): A_t =
                       [W0(t, in 0..din/32-1)], B_t = [W1(0..ceil(dout/32)-1, t)]; used when dout <= 64 (else the
                       launch needs W).  With it W may be NULL. */
  const void* Wh;   /* optional fp16 two-part image of the same stream (f16x3 path; needs Wx too) */
} gn_mlp2_group_t;
int gn_mlp2_f32(const gn_mlp2_group_t* groups, int n_groups, int rows, int din, int dh, int dout, int ldy,
                int N, float divisor, gn_stream_t stream);
/* twin: dout <= 64 */
int gn_mlp2_bf16(const gn_mlp2_group_t* groups, int n_groups, int rows, int din, int dh, int dout, int ldy,
                 int N, float divisor, gn_stream_t stream);

/* ---- launch plans (ABI 36; the graph stage and the scatter: ABI 38) ------------------------------
 * What a forward launcher would launch for its arguments, without launching: every launcher below is "plan, then launch",
 * and gn_*_plan_* return the plan alone.  A plan is decided on the host from the descriptors, the scalar arguments, the
 * storage type and the per-call environment switches (GN_XCD, GN_POOL_STAGE, GN_AGG_LINES, GN_AGG_HSTAGE, GN_AGG_RB2,
 * GN_EDGE_RB2, GN_RB2_MIN_PAIRS, GN_MLP2_XS, GN_N2E_ROWS, GN_SCATTER_PAIRS; read once per call): no HIP call, no GPU needed,
 * device addresses are only tested for NULL and alignment (a not yet allocated output may be any aligned non-NULL
 * placeholder).  The return value is the launcher's for the same arguments; on an error the plan's content is unspecified.
 * Per-group arrays are in the caller's group order.
 * The graph stage (ABI 38): gn_affinity_f32, gn_topk_incidence_f32 and gn_affinity_topk_* are planned the same way (plans
 * without groups: kernel, grid, dyn_lds).  The fused job's argument checks and its scene tile are stated once, for
 * gn_affinity_topk_*'s plan (against the 128 KiB budget of a workgroup) and the node stage's tail (against
 * gn_affinity_tail_lds_limit(), no masks) alike: which of the three forms builds a graph — tail, fused launch, or the
 * banded pair — is what gn_node_mlp_plan_* and gn_affinity_topk_plan_* answer (GN_OK or GN_ERR_LDS). */
#define GN_K_NONE 0                  /* no main launch (every group ran in a launch of its own, see pre_kernel) */
#define GN_K_NODE_STAGE 1
#define GN_K_NODE_MLP_SPLIT 2
#define GN_K_NODE_MLP 3
#define GN_K_EDGE_X 4
#define GN_K_EDGE_RB2 5
#define GN_K_EDGE_MLP_GUMBEL 6
#define GN_K_AGG_X 7
#define GN_K_AGG_RB2 8
#define GN_K_AGG_MLP 9
#define GN_K_MLP2_XS 10
#define GN_K_MLP2_X 11
#define GN_K_MLP2_SPLIT 12
#define GN_K_MLP2 13
#define GN_K_NODE2EDGE 14
#define GN_K_AGG_GATHER 15
#define GN_K_AGG_GATHER_MASK 16      /* the gather of groups with rowmask (ABI 37) */
/* ABI 38: the kernels of the launches of their own (pre_kernel) and of the graph stage and the scatter */
#define GN_K_AGG_SCENE 17            /* typed aggregation, bf16 storage: the pairwise group's scene form */
#define GN_K_AGG_GATHER_PAIRWISE 18  /* gather of a pairwise group */
#define GN_K_AFFINITY_TOPK 19        /* fused affinity + top-k, one workgroup per scene (gn_affinity_f32: without scales) */
#define GN_K_AFFINITY_TOPK_MASKS 20  /* ... that also emits the bit-mask form */
#define GN_K_AFFINITY_BANDED 21      /* gn_affinity_f32 beyond the fused tile: 16-row bands against 64-column panels */
#define GN_K_TOPK_INCIDENCE 22
#define GN_K_AGG_SCATTER 23          /* staged scatter of the hyper groups: G scenes per workgroup */
#define GN_K_AGG_SCATTER_MASK 24     /* ... of groups with colmask */
#define GN_K_AGG_SCATTER_DIRECT 25   /* scatter of one group from global memory (its mode is the group's: H, ordered pairs
                                        or, sym, unordered pairs) */
#define GN_K_AGG_SCATTER_PAIRS 26    /* scatter of the unordered pairs, one workgroup per scene */
/* ABI 39: the kernels of the ragged entry points */
#define GN_K_AFFINITY_TOPK_RAGGED 27
#define GN_K_TOPK_INCIDENCE_RAGGED 28
#define GN_K_NODE2EDGE_RAGGED 29     /* variant: 0 banded, 1 row form, as GN_K_NODE2EDGE */
#define GN_K_AGG_SCATTER_RAGGED 30   /* grid (ceil(B N 32 / 256) capped, groups) */
#define GN_K_ZERO_PADDING 31         /* grid (capped, items); a plan without groups */
/* additions within ABI 40: the kernels of the subset route, in a range of their own — the table above ends at
 * GN_K_ZERO_PADDING as it did (callers may rely on gn_kernel_name(32) == NULL); ids 32..39 name no kernel */
#define GN_K_AGENT_SUBSET 40         /* grid (ceil(B / 4)): one wave per scene */
#define GN_K_REMAP_ROWS 41           /* grid (capped, items) */
typedef struct {
  int kernel;        /* GN_K_*: the kernel of the launch (gn_kernel_name), instantiated for ... */
  int precision;     /* ... 0: the plain fp32 weight stream, 1: bf16 storage (the twins), 2: f16x3, 3: bf16x6 */
  int variant;       /* ... agg_x_kernel: 1 = with the per-pair forms of the pairwise graph; node2edge_kernel: 1 = row form
                        (0 = banded), 2 = row form reading member words (gn_node2edge_masks_*; see SGh, EBh) */
  int tiles[3];      /* ... closing MLP: 32-wide tiles (IT, HT, OT) of din, dh and dout (OT = 0: any dout) */
  int grid[3];       /* workgroups of the launch (x with XCD order: 8 x the largest per-XCD share) */
  int dyn_lds;       /* dynamic LDS bytes of the launch */
  int stage_bytes;   /* LDS stage the kernel is told: edge kernels the pool stage (-1 = GN_POOL_STAGE off), agg_rb2_kernel the
                        staged ori rows */
  int xcd;           /* 1: workgroups dealt over the XCDs section by section */
  int closing;       /* typed aggregation: 1 = the launch carries the fused closing stage (gn_agg_group_t.y) */
  int n_groups;
  int wgs[GN_MAX_GROUPS];         /* workgroups of the group in the launch (0 for a group launched on its own) */
  int wpr[GN_MAX_GROUPS];         /* typed aggregation: waves per 32-row block */
  int spw[GN_MAX_GROUPS];         /* fused closing stage: scenes per workgroup (0: none) */
  int stage[GN_MAX_GROUPS];       /* pair form: per-node pre-activations staged in LDS */
  int lines[GN_MAX_GROUPS];       /* fused hyper gather: 0 per lane, 1 line layout, 2 from staged ori rows */
  int node_form[GN_MAX_GROUPS];   /* node form (bf16 storage without A: the scene form, in a launch of its own) */
  int unstaged[GN_MAX_GROUPS];    /* edge_x_kernel: hyper group pooled without a stage, one workgroup per 32-row block */
  int pos[GN_MAX_GROUPS];         /* the group's position in the launch (typed aggregation: after the cost sort), -1 when
                                     it is not part of it */
  int pre_grid[GN_MAX_GROUPS];    /* > 0: the group runs in a launch of its own ahead of the main one, with this grid ... */
  int pre_lds[GN_MAX_GROUPS];     /* ... and this dynamic LDS ... */
  int SGh, EBh;      /* node -> edge: scenes per workgroup and hyperedges per band of the hyper groups (row form: EBh = 0; so is variant
                        2, whose plan equals variant 1's in every other field) */
  int G, TE;         /* gather: scenes per workgroup and hyperedges per tile (mask form: TE = the largest E, one tile);
                        scatter: scenes per workgroup and TE = the largest E of the staged groups (one tile);
                        gn_topk_incidence_f32 reuses TE for the rows of corr per band (grid[0] bands of TE rows) */
  int pre_kernel[GN_MAX_GROUPS];  /* ... of this kernel (GN_K_*; ABI 38, GN_K_NONE where pre_grid is 0) */
} gn_launch_plan_t;
/* "agg_x_kernel", ...: the kernel's name as a kernel trace shows it (without template arguments); NULL for an unknown id */
const char* gn_kernel_name(int kernel);
/* job may be NULL: gn_node_mlp_* without, gn_node_mlp_affinity_* with the affinity tail */
int gn_node_mlp_plan_f32(const gn_node_group_t* groups, int n_groups, int rows, const gn_affinity_job_t* job,
                         gn_launch_plan_t* plan);
int gn_node_mlp_plan_bf16(const gn_node_group_t* groups, int n_groups, int rows, const gn_affinity_job_t* job,
                          gn_launch_plan_t* plan);
/* static_lds: the static LDS of the launch's kernel, which bounds the pool stage and which only the HIP runtime knows;
 * negative = ask the runtime (what the launcher does; needs a GPU) */
int gn_edge_mlp_gumbel_plan_f32(const gn_edge_group_t* groups, int n_groups, float tau, unsigned long long seed,
                                const unsigned long long* offset_dev, long long static_lds, gn_launch_plan_t* plan);
int gn_edge_mlp_gumbel_plan_bf16(const gn_edge_group_t* groups, int n_groups, float tau, unsigned long long seed,
                                 const unsigned long long* offset_dev, long long static_lds, gn_launch_plan_t* plan);
int gn_agg_mlp_plan_f32(const gn_agg_group_t* groups, int n_groups, gn_launch_plan_t* plan);
int gn_agg_mlp_plan_bf16(const gn_agg_group_t* groups, int n_groups, gn_launch_plan_t* plan);
int gn_mlp2_plan_f32(const gn_mlp2_group_t* groups, int n_groups, int rows, int din, int dh, int dout, int ldy, int N,
                     float divisor, gn_launch_plan_t* plan);
int gn_mlp2_plan_bf16(const gn_mlp2_group_t* groups, int n_groups, int rows, int din, int dh, int dout, int ldy, int N,
                      float divisor, gn_launch_plan_t* plan);
int gn_node2edge_plan_f32(const gn_n2e_group_t* groups, int n_groups, int B, int N, gn_launch_plan_t* plan);
int gn_node2edge_plan_bf16(const gn_n2e_group_t* groups, int n_groups, int B, int N, gn_launch_plan_t* plan);
int gn_node2edge_masks_plan_f32(const gn_n2e_group_t* groups, const unsigned long long* const* rowmasks, int n_groups,
                                int B, int N, gn_launch_plan_t* plan);
int gn_node2edge_masks_plan_bf16(const gn_n2e_group_t* groups, const unsigned long long* const* rowmasks, int n_groups,
                                 int B, int N, gn_launch_plan_t* plan);
int gn_agg_gather_plan_f32(const gn_gather_group_t* groups, int n_groups, int B, int N, gn_launch_plan_t* plan);
int gn_agg_gather_plan_bf16(const gn_gather_group_t* groups, int n_groups, int B, int N, gn_launch_plan_t* plan);
/* The scatter (ABI 38).  A group in the staged (or mask) launch: pos / wgs / spw = G as in the gather's plan, kernel, grid =
 * (ceil(B / G), staged groups), G, TE, dyn_lds.  A group launched on its own, in group order ahead of the staged launch:
 * pos = -1, pre_kernel (the pairs kernel for sym groups with 16 N <= 1024 and B >= 256 unless GN_SCATTER_PAIRS = 0, else the
 * direct kernel, which also takes a hyper group whose E (64 + N) floats exceed 64 KiB) and pre_grid. */
int gn_agg_scatter_plan_f32(const gn_scatter_group_t* groups, int n_groups, int B, int N, float divisor,
                            gn_launch_plan_t* plan);
int gn_agg_scatter_plan_bf16(const gn_scatter_group_t* groups, int n_groups, int B, int N, float divisor,
                             gn_launch_plan_t* plan);
/* The graph stage (ABI 38): n_groups = 0.  gn_affinity_plan_f32: GN_K_AFFINITY_TOPK with grid (B) and the fused tile, or
 * GN_K_AFFINITY_BANDED with grid (ceil(N / 16), B).  gn_topk_incidence_plan_f32: grid (bands, B), TE rows per band.
 * gn_affinity_topk_plan_*: grid (B), dyn_lds = the scene tile; GN_ERR_LDS where the caller takes the banded pair. */
int gn_affinity_plan_f32(const float* f, float* corr, int B, int N, int D, gn_launch_plan_t* plan);
int gn_topk_incidence_plan_f32(const float* corr, float* const* H_list, const int* k_list, int n_scales, int B, int N,
                               gn_launch_plan_t* plan);
int gn_affinity_topk_plan_f32(const float* f, float* corr, float* const* H_list, const int* k_list, int n_scales, int B,
                              int N, int D, const gn_block_extras_t* extras, unsigned long long* const* rowmask_list,
                              unsigned long long* const* colmask_list, gn_launch_plan_t* plan);
int gn_affinity_topk_plan_bf16(const void* f, float* corr, float* const* H_list, const int* k_list, int n_scales, int B,
                               int N, int D, const gn_block_extras_t* extras, unsigned long long* const* rowmask_list,
                               unsigned long long* const* colmask_list, gn_launch_plan_t* plan);

/* The ragged entry points (ABI 39): the plans of their full-batch counterparts with the kernel ids above; n_valid is
 * tested for NULL and 4-byte alignment like every other address. */
int gn_affinity_topk_ragged_plan_f32(const float* f, float* corr, float* const* H_list, const int* k_list, int n_scales,
                                     int B, int N, int D, const gn_block_extras_t* extras, const int* n_valid,
                                     gn_launch_plan_t* plan);
int gn_affinity_topk_ragged_plan_bf16(const void* f, float* corr, float* const* H_list, const int* k_list, int n_scales,
                                      int B, int N, int D, const gn_block_extras_t* extras, const int* n_valid,
                                      gn_launch_plan_t* plan);
int gn_topk_incidence_ragged_plan_f32(const float* corr, float* const* H_list, const int* k_list, int n_scales, int B,
                                      int N, const int* n_valid, gn_launch_plan_t* plan);
int gn_node2edge_ragged_plan_f32(const gn_n2e_group_t* groups, int n_groups, int B, int N, const int* n_valid,
                                 gn_launch_plan_t* plan);
int gn_node2edge_ragged_plan_bf16(const gn_n2e_group_t* groups, int n_groups, int B, int N, const int* n_valid,
                                  gn_launch_plan_t* plan);
int gn_agg_scatter_ragged_plan_f32(const gn_scatter_group_t* groups, int n_groups, int B, int N, float divisor,
                                   const int* n_valid, gn_launch_plan_t* plan);
int gn_agg_scatter_ragged_plan_bf16(const gn_scatter_group_t* groups, int n_groups, int B, int N, float divisor,
                                    const int* n_valid, gn_launch_plan_t* plan);
int gn_zero_padding_plan(const gn_zero_item_t* items, int n_items, int B, int N, const int* n_valid,
                         gn_launch_plan_t* plan);
/* The two launches of ABI 40.  Their kernels have no GN_K_* id (the table above is unchanged): kernel = GN_K_NONE,
 * grid = (ceil(B / 4)) for the counts — one wave per scene, four to a workgroup — and (capped, items) for the zeroing. */
int gn_zero_empty_scenes_plan(const gn_zero_item_t* items, int n_items, int B, const int* n_valid, gn_launch_plan_t* plan);
int gn_agent_counts_plan_u8(const unsigned char* valid, int B, int N, int* n_valid, unsigned int* status,
                            gn_launch_plan_t* plan);
/* The subset route's two launches (additions within ABI 40).  gn_agent_subset_plan: kernel = GN_K_AGENT_SUBSET, grid =
 * (ceil(B / 4)).  gn_remap_rows_plan: kernel = GN_K_REMAP_ROWS, grid = (capped, items), n_groups = min(n_items,
 * GN_MAX_GROUPS), stage[g] = the store unit in bytes (16 / 8 / 4 / 2) of item g for g < GN_MAX_GROUPS, stage_bytes = the
 * smallest store unit over all items. */
int gn_agent_subset_plan(const unsigned char* valid, int B, int N, int* n_valid, int* order, int* slot, unsigned int* status,
                         gn_launch_plan_t* plan);
int gn_remap_rows_plan(const gn_remap_item_t* items, int n_items, int B, int N, const int* map, gn_launch_plan_t* plan);

/* ---- backward (training) building blocks — SURVEY.md §8f rank 2 -------------------------------
 * train_hyper_nba.py:116 back-propagates through the two modules.  The backward of the path is
 * assembled (groupnet_amd/backward.py) from these generic kernels plus the forward gather / scatter
 * kernels, which are each other's adjoints.  All pointers device fp32, row-major.
 *
 * gn_gemm_f32: C (M x N, ldc) = beta*C + alpha*op(A) op(B) [+ bias[n]] [relu] [zeroed where mask[m][n] <= 0];
 *   op(A) = A (M x K, lda) or, transA, A^T with A stored (K x M, lda); op(B) = B (K x N, ldb) or, transB,
 *   B^T with B stored (N x K, ldb).  With few output tiles and K >= 4096 (weight gradients dW = dY^T X)
 *   K is split over workgroups and partial sums are added atomically (then no bias/relu/mask).
 * gn_gumbel_bwd_f32: back through edge_feat = sigmoid(f) * dist, dist = softmax((logits + g)/tau)
 *   (model/MS_HGNN_batch.py:45-50): dist (rows,K), lgf (rows,ldl) whose column K is f, def = d edge_feat,
 *   gdist = d dist or NULL -> dlgf (rows,ldl): columns 0..K-1 = d logits, column K = d f, rest 0.
 *   sym_N > 0 (here and in gn_gumbel_ef_f32): the rows of lgf / def / dlgf / ef are the N(N+1)/2 unordered
 *   pairs of the pairwise graph per scene, dist / gdist stay per ordered edge (B, N*N, K): a pair row
 *   stands for the ordered edges (i,j) and (j,i) — ef is their sum (self-loop rows times diag_w: 2 gives the
 *   rows the forward's pair-form aggregation consumes, which fold H = 2 into ef), dlgf the sum of their
 *   gradients.
 * gn_node2edge_bwd_f32: back through gn_node2edge_f32 for an explicit H (B,E,N), or H == NULL for the
 *   implicit pairwise graph (E == N*N ordered edges, or with sym its N(N+1)/2 unordered pairs whose dedges
 *   are already summed over the two directions): given dedges (B,E,64) ADDS into dxp (B,N,64),
 *   dpq (B,N,64), dw2 (32), db2 (1) (zero them first).  One workgroup per scene with the scene's rows in
 *   LDS while they fit (N <= ~140); beyond that one wave per hyperedge with global atomics (explicit H only). */
/* Grouped form: n independent problems in one launch (all types of the typed aggregation MLP, all modules
 * of a multiscale block).  rs (optional) scales A's STORED rows: A_eff[r][:] = rs[r*rs_ld] * A[r][:];
 * colsum (optional, GN_GEMM_TRANS_A only) receives colsum[m] += sum_k A_eff[k][m] — the bias gradient next
 * to dW = dY^T X.  GN_GEMM_ACCUM: C += alpha*op(A)op(B) by atomic adds with K split over workgroups (C must
 * hold zeros / the running sum; no bias, relu, mask, beta). */
#define GN_GEMM_TRANS_A 1
#define GN_GEMM_TRANS_B 2
#define GN_GEMM_RELU 4
#define GN_GEMM_ACCUM 8
#define GN_GEMM_TRANS_C 16   /* with GN_GEMM_ACCUM: the product is added into C^T, i.e. C is (N x M, ldc) */
typedef struct {
  const float* A;
  const float* B;
  float* C;
  const float* bias;
  const float* mask;
  const float* rs;
  float* colsum;
  int M, N, K, lda, ldb, ldc, ldmask, rs_ld;
  int flags;
  float alpha, beta;
} gn_gemm_desc_t;
int gn_gemm_grouped_f32(const gn_gemm_desc_t* descs, int n, gn_stream_t stream);
int gn_gemm_f32(const float* A, const float* B, float* C, int M, int N, int K, int lda, int ldb, int ldc,
                int transA, int transB, const float* bias, const float* mask, int ldmask, int relu,
                float alpha, float beta, gn_stream_t stream);
/* The ordered (deterministic) form of the grouped launch (additions within ABI 40): the same descriptors, and a result
 * that is bit-identical from run to run.
 *   - A problem without GN_GEMM_ACCUM has one writer per element already: it runs as in gn_gemm_grouped_f32 and returns
 *     its bits.
 *   - An accumulate problem keeps gn_gemm_grouped_f32's form — the staging kernel (vector: A, B 16-byte aligned, lda,
 *     ldb multiples of 4, K a multiple of 32, M (transA) / N (not transB) multiples of 4; else scalar), the tiles and the
 *     split rule: with t = ceil(M/128) ceil(N/64) tiles, s0 = min(ceil(512/t), ceil(K/256)),
 *     kchunk = ceil(ceil(K/s0)/32) 32, splits = ceil(K/kchunk); split s covers k in [s kchunk, min(K, (s+1) kchunk)).
 *     Each (tile, split) workgroup stores its alpha-scaled partial tile — the value the atomic form would add — to the
 *     caller's workspace at part[s][row][col] (dense, C's orientation) and, where colsum is set, its partial column sums
 *     at cs_part[s][m], by plain stores.  A second kernel of the same call then forms, per destination element,
 *         v = C_old;  for s = 0 .. splits-1:  v = v + part[s];  C = v
 *     in fp32, one thread per element, and colsum[m] the same way from cs_part.
 *   - Accumulate problems of one call with the IDENTICAL destination (the same C, ldc, M, N and GN_GEMM_TRANS_C; or the
 *     same colsum and M) form a chain: their partials are added in descriptor order, split order within each, into the
 *     one running v.  Accumulate destinations (C's and colsums) that share an element without being identical:
 *     GN_ERR_SHAPE, nothing launched (the same ld: decided per element, so column slices of one matrix pass; different
 *     ld with intersecting address ranges: refused).
 *   - A problem's result depends on its own descriptor alone (shapes, leading dimensions, flags, alignment, values),
 *     not on the other problems of the call, its position, the device's size or the environment.
 *   - n <= GN_GEMM_DET_MAX, else GN_ERR_SHAPE.  workspace: device memory, 16-byte aligned (GN_ERR_ALIGN), at least
 *     gn_gemm_grouped_det_plan's workspace_bytes (GN_ERR_SHAPE), NULL only where that is 0 (GN_ERR_NULL); its content
 *     before and after the call is of no interest.  The launcher never allocates.
 * gn_gemm_grouped_det_plan: pure host arithmetic — per problem splits, kchunk, the staging kernel, the chain (the index of
 * the first problem of the call with its destination; -1: not an accumulate problem), the same for colsum (-1: none), the
 * byte offsets of part and cs_part in the workspace (-1: none), and the workspace's size; returns what the launcher
 * returns for the same descriptors (the workspace apart). */
#define GN_GEMM_DET_MAX 128
#define GN_GEMM_KERNEL_SCALAR 0
#define GN_GEMM_KERNEL_VECTOR 1
typedef struct {
  long long workspace_bytes;
  int n;
  int n_chains;
  int splits[GN_GEMM_DET_MAX];
  int kchunk[GN_GEMM_DET_MAX];
  int kernel[GN_GEMM_DET_MAX];
  int chain[GN_GEMM_DET_MAX];
  int cs_chain[GN_GEMM_DET_MAX];
  long long offset[GN_GEMM_DET_MAX];
  long long cs_offset[GN_GEMM_DET_MAX];
} gn_gemm_det_plan_t;
int gn_gemm_grouped_det_f32(const gn_gemm_desc_t* descs, int n, void* workspace, size_t workspace_bytes,
                            gn_stream_t stream);
int gn_gemm_grouped_det_plan(const gn_gemm_desc_t* descs, int n, gn_gemm_det_plan_t* plan);
/* out (rows x cols, ldo) = alpha * a (rows x cols, lda) + beta * out — slices, scalings and sums of
 * gradients without leaving the library. */
int gn_axpby2d_f32(float* out, int ldo, const float* a, int lda, long long rows, int cols, float alpha,
                   float beta, gn_stream_t stream);
/* ef[r][k] = sigmoid(lgf[r][K]) * dist[r][k]: edge_feat of MLP_dict_softmax from dist and the factor
 * pre-activation (column K of lgf (rows, ldl)); ef has leading dimension ld_ef >= K (a multiple of 4 keeps
 * the GEMMs that read it on the vector path). */
int gn_gumbel_ef_f32(const float* dist, const float* lgf, float* ef, long long rows, int K, int ldl, int sym_N,
                     float diag_w, int ld_ef, gn_stream_t stream);
/* Middle of the typed aggregation MLP's backward (model/MS_HGNN_batch.py:264-265), all K types of a row at
 * once: T (rows, K*hid) holds dfeat W2cat, Hc (rows, K*hid) the hidden activations; writes
 * def[r][k] = <T[r,k,:], Hc[r,k,:]> + <dfeat[r], b2[k]> and T[r,k,:] <- ef[r][k] * T[r,k,:] * (Hc > 0). */
int gn_typed_bwd_f32(float* T, const float* Hc, const float* ef, int ld_ef, const float* dfeat, const float* b2,
                     float* def, long long rows, int K, int hid, gn_stream_t stream);
int gn_gumbel_bwd_f32(const float* dist, const float* lgf, const float* def, const float* gdist, float* dlgf,
                      long long rows, int K, int ldl, float tau, int sym_N, gn_stream_t stream);
/* The two per-module stages above for every module of a backward round in ONE launch each (descriptor arrays in HOST
 * memory, 1 <= n_groups <= GN_MAX_GROUPS; all modules over the same B scenes and N nodes): the single-module launches
 * take 13-88 us each and ran end to end, four per stage and training step.  gn_node2edge_bwd_grouped_f32 covers the
 * per-scene form only (the scene's rows fit in LDS, else GN_ERR_LDS: go module by module). */
typedef struct {
  const float* dist;
  const float* lgf;
  const float* def;
  const float* gdist;   /* or NULL */
  float* dlgf;
  long long rows;
  int K;
  int sym_N;
} gn_gumbel_bwd_group_t;
int gn_gumbel_bwd_grouped_f32(const gn_gumbel_bwd_group_t* groups, int n_groups, int ldl, float tau, gn_stream_t stream);
typedef struct {
  const float* xp;
  const float* pq;
  const float* H;       /* or NULL: the pairwise graph */
  const float* w2;
  const float* b2;
  const float* dedges;
  float* dxp;
  float* dpq;
  float* dw2;
  float* db2;
  int E;
  int sym;
} gn_n2e_bwd_group_t;
int gn_node2edge_bwd_grouped_f32(const gn_n2e_bwd_group_t* groups, int n_groups, int B, int N, gn_stream_t stream);
int gn_node2edge_bwd_f32(const float* xp, const float* pq, const float* H, const float* w2, const float* b2,
                         const float* dedges, float* dxp, float* dpq, float* dw2, float* db2, int B, int N,
                         int E, int sym, gn_stream_t stream);
/* The same two launches over a ragged batch (header comment, "Ragged batches"; additions within ABI 40): back through
 * gn_node2edge_ragged_f32.  The arguments of their counterparts plus n_valid (validated as everywhere: GN_ERR_NULL /
 * GN_ERR_ALIGN), the same in-out convention.  Scene b, n_b = n_valid[b] clamped to [0, N]: the softmax of a hyperedge
 * runs over the scene's n_b nodes (n_b - members non-members, the 0 in the running maximum only where one exists); an
 * explicit H is read at its columns n < n_b (the ragged incidences are zero beyond) and a row without members there is
 * skipped; a pairwise group walks the pairs with both ends < n_b and reads dedges at their PADDED rows (i*N + j, or the
 * unordered row of (i, j) at size N).  Rows n >= n_b of dxp and dpq are neither read nor written; a scene with
 * n_b == 0 adds nothing anywhere.  The per-scene form only — one workgroup per scene, the padded scene's LDS request
 * (4 N 64 + 64 + 16 N) 4 B — so N > 140 is GN_ERR_LDS and nothing is launched. */
int gn_node2edge_bwd_ragged_grouped_f32(const gn_n2e_bwd_group_t* groups, int n_groups, int B, int N,
                                        const int* n_valid, gn_stream_t stream);
int gn_node2edge_bwd_ragged_f32(const float* xp, const float* pq, const float* H, const float* w2, const float* b2,
                                const float* dedges, float* dxp, float* dpq, float* dw2, float* db2, int B, int N,
                                int E, int sym, const int* n_valid, gn_stream_t stream);
/* The ordered (deterministic) form of the grouped per-scene launch (addition within ABI 40), full-batch (n_valid == NULL)
 * or ragged (n_valid: the device counts, validated and clamped as above; a scene with n_b == 0 adds nothing).  One WAVE
 * per (scene, module) walks the scene's edges in ascending order — rows of an explicit H, or the pairs in the order (and
 * with the ragged addressing) of the default form — and adds each edge's contributions to the scene's dxp / dpq rows in
 * LDS by plain read-modify-writes, every address owned by one lane: a row's sum is start + edge 0 + edge 1 + ..., the
 * scene's rows then added once to dxp / dpq as before.  The 33 sums of attention layer 1 of (module g, scene b) go to
 * partials[(g B + b) 33 ..] (32 of dw2, then db2; an empty scene writes zeros) by plain stores, and a second kernel of the
 * same call forms dw2[c] = dw2_old[c] + partial(b = 0)[c] + partial(1)[c] + ... in ascending scene order, db2 likewise.
 * partials: n_groups B 33 floats of device memory (NULL: GN_ERR_NULL; 4-byte aligned, else GN_ERR_ALIGN), content of no
 * interest before or after.  The per-scene form only, with the default form's limit: N > 140 is GN_ERR_LDS and nothing
 * is launched. */
int gn_node2edge_bwd_det_grouped_f32(const gn_n2e_bwd_group_t* groups, int n_groups, int B, int N, const int* n_valid,
                                     float* partials, gn_stream_t stream);

/* ---- device noise (build's own; the reference draws torch.rand on the host) --------------------
 * U[i] = Philox4x32-10(counter = (i + offset) / 4, key = seed)[(i + offset) % 4] >> 8, scaled to
 * [0,1).  Lets a sharded run draw exactly the rows of the full-batch stream it owns.
 * offset_dev (may be NULL): a device counter ADDED to `offset` when the kernel runs, so that a
 * captured hipGraph draws fresh noise on every replay; gn_counter_add_u64 advances it in stream
 * order. */
int gn_philox_uniform_f32(float* U, size_t n, unsigned long long seed, unsigned long long offset,
                          const unsigned long long* offset_dev, gn_stream_t stream);
int gn_counter_add_u64(unsigned long long* counter, unsigned long long add, gn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* GROUPNET_HIP_H */
