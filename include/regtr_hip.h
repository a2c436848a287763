/*
 * regtr_hip.h -- C ABI of libregtr_hip.so: the gfx950 (MI355X) kernels of the RegTR correspondence-inference hot
 * path.  Plain pointers and sizes only, no torch types: any host (ctypes, cgo, JNI, a C++ pipeline) can bind it.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless its comment says "host";
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); all work is enqueued, nothing synchronises;
 *   - return value: 0 = OK, <0 = error (REGTR_ERR_*); nothing throws across the boundary.  The Python shim raises
 *     RuntimeError on a non-zero status, as the reference's CPython wrappers do
 *     (cpp_neighbors/wrapper.cpp:77,95,133,203);
 *   - clouds of a batch are STACKED: rows [seg_off[c], seg_off[c+1]) belong to cloud c; seg_off is int32 [n_clouds+1]
 *     ON THE DEVICE so that data-dependent level sizes never have to visit the host between kernels.  `*_cap`
 *     arguments are host-known upper bounds used only to size launches and buffers.
 *   - indices are int32; the shadow / pad index is the total number of support rows (neighbors.cpp:323-324).
 *
 * Reference interfaces replaced (paths relative to /root/reference/src):
 *   regtr_grid_subsample      cpp_subsampling.subsample_batch     models/backbone_kpconv/cpp_wrappers/cpp_subsampling/wrapper.cpp:62-333
 *                             = batch_grid_subsampling            .../grid_subsampling/grid_subsampling.cpp:109-211
 *                             (GPU twin batch_grid_subsampling_kpconv_gpu, models/backbone_kpconv/kpconv.py:213-240)
 *   regtr_cellgrid_build +
 *   regtr_radius_query        cpp_neighbors.batch_query           .../cpp_neighbors/wrapper.cpp:58-238
 *                             = batch_nanoflann_neighbors         .../cpp_neighbors/neighbors/neighbors.cpp:211-332
 *                             (GPU twin batch_neighbors_kpconv_gpu, kpconv.py:261-288)
 *   regtr_kpconv_gather +
 *   regtr_gemm_f32            KPConv.forward                      models/backbone_kpconv/kpconv_blocks.py:269-414
 *   regtr_maxpool_gather      max_pool                            kpconv_blocks.py:127-143
 *   regtr_instnorm_*          BatchNormBlock (InstanceNorm1d) + LeakyReLU + residual   kpconv_blocks.py:497-519,556-561,741
 *   regtr_gemm_f32 / _x3 /
 *   regtr_gemm_stream         nn.Linear call sites                kpconv_blocks.py:557, regtr.py:145,432-436, transformers.py:197-238
 *   regtr_block_tail          ResnetBottleneckBlock tail (unary2 + unary_shortcut + sum + LeakyReLU), SimpleBlock after its gather
 *                                                                 kpconv_blocks.py:727-741, 590-646
 *   regtr_encoder_fwd         KPFEncoder.forward (blocks sequenced) models/backbone_kpconv/kpconv.py:81-88, kpconv_blocks.py:632-646,706-741
 *   regtr_layernorm           nn.LayerNorm (+ with_pos_embed)     transformers.py:116-119,194-195,213-215,232
 *   regtr_posemb_sine         PositionEmbeddingCoordsSine.forward models/transformer/position_embedding.py:29-50
 *   regtr_posemb_mlp          PositionEmbeddingLearned.forward    models/transformer/position_embedding.py:53-72
 *   regtr_mha_fwd             nn.MultiheadAttention core          transformers.py:197-226
 *   regtr_attn_xyz            CorrespondenceDecoder.simple_attention   models/regtr.py:316-351
 *   regtr_weighted_procrustes pose assembly + compute_rigid_transform   regtr.py:185-203, utils/se3_torch.py:108-154
 *   regtr_weighted_procrustes_bwd  its backward (what autograd gives the reference through torch.svd)   the same lines
 *   regtr_infonce             InfoNCELossFull.compute_infonce     models/losses/feature_loss.py:281-314
 *   regtr_se3_transform       se3_transform (GT overlap masks)    data_loaders/threedmatch.py:78-84
 *   regtr_loss_terms          overlap BCE + CorrCriterion sums    models/regtr.py:250-285, models/losses/corr_loss.py:18-40
 *   regtr_infonce_rows / _bwd InfoNCELossFull forward + backward  models/losses/feature_loss.py:246-314
 *   regtr_gemm_tn             dW of InfoNCELossFull (G^T dP')     models/losses/feature_loss.py:295-297
 *   regtr_corr_l1_bwd         CorrCriterion('mae') backward       models/losses/corr_loss.py:24-37
 *   regtr_circle_rows / _bwd  CircleLossFull ('euclidean') forward + backward   models/losses/feature_loss.py:160-243
 *   regtr_mha_bwd             nn.MultiheadAttention core, backward   transformers.py:197-226
 *   regtr_layernorm_bwd       nn.LayerNorm backward (+ the residual branch's gradient)   transformers.py:194-238
 *   regtr_bias_relu_bwd       nn.Linear bias gradient, F.relu backward   transformers.py:194-238
 *   regtr_nbr_transpose       the neighbour table by support (what autograd's index backward scatters through)   kpconv_blocks.py:312,391
 *   regtr_kpconv_gather_bwd   KPConv.forward backward, input features    kpconv_blocks.py:309-394
 *   regtr_row_div             KPConv.forward backward, the neighbour-count normaliser   kpconv_blocks.py:409-412
 *   regtr_gemm_tn_any         KPConv.forward backward, weights (WF^T g) at widths regtr_gemm_tn refuses   kpconv_blocks.py:401-406
 *   regtr_instnorm_bwd        BatchNormBlock (InstanceNorm1d) + LeakyReLU + shortcut, backward   kpconv_blocks.py:497-519,556-561,741
 *   regtr_maxpool_argmax      max_pool: the index torch.max(dim) keeps for autograd   kpconv_blocks.py:142
 *   regtr_maxpool_fwd_argmax  max_pool and that index in one pass over the rows               kpconv_blocks.py:127-143
 *   regtr_maxpool_gather_bwd  max_pool backward                   kpconv_blocks.py:127-143
 *   regtr_head_tail_bwd       CorrespondenceRegressor backward, the 3-wide and 1-wide output Linears   models/regtr.py:432-441
 *   regtr_bce_logits_bwd      nn.BCEWithLogitsLoss backward (the overlap loss)   models/regtr.py:250-257
 *   regtr_cloud_centroids +
 *   regtr_augment_draws       RigidPerturb, RandomSwap (the decisions and the poses)   data_loaders/transforms.py:15-72,132-149
 *   regtr_shuffle_keys +
 *   regtr_augment_gather      RigidPerturb, Jitter, ShufflePoints, RandomSwap (the points and masks)   data_loaders/transforms.py:58-149
 *   regtr_modelnet_draws      uniform_2_sphere, RandomTransformSE3_euler (the decisions and the pose)   data_loaders/modelnet_transforms.py:18-43,316-355
 *   regtr_crop_select         RandomCrop.crop (a per-cloud percentile by radix select)   data_loaders/modelnet_transforms.py:188-200
 *   regtr_modelnet_keys +
 *   regtr_modelnet_gather     Resampler, RandomJitter, ShufflePoints, the crop's overlap masks   data_loaders/modelnet_transforms.py:63-173,219-228,374-397
 *   regtr_nearest +
 *   regtr_segment_mean        the modified Chamfer distance (nearest neighbours, per-cloud means)   benchmark/benchmark_modelnet.py:69-76
 *   regtr_pose_metrics        se3_compare; the RPMNet / DCP pose metrics   utils/se3_torch.py:93-105, benchmark/benchmark_modelnet.py:51-67
 *   regtr_gather_segments     (no reference counterpart) packs the cached per-cloud tokens of the pairs of one RegTR.register call
 *   regtr_icp_step            (no reference counterpart) one point-to-point ICP iteration on the raw clouds: fused transform + nearest
 *                             match + float64 moments, then the per-pair Kabsch solve, fitness / inlier_rmse and the stop rule
 *   regtr_icp_ws_bytes /
 *   regtr_icp_chunk           (no reference counterpart) its workspace size and chunking
 *   regtr_estimate_normals    (no reference counterpart) per-point surface normals from the exact integer moments of the radius neighbourhood
 *   regtr_icp_plane_step      (no reference counterpart) one point-to-plane ICP iteration: regtr_icp_step's match, the 6x6 normal
 *                             equations in float64, the LDL^T solve and the update of a float64 master pose
 */
#ifndef REGTR_HIP_H
#define REGTR_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define REGTR_OK 0
#define REGTR_ERR_LAUNCH (-1)
#define REGTR_ERR_ARG (-2)
#define REGTR_ERR_WORKSPACE (-3)

/* ABI version of THIS header.  Entry points have gained arguments between versions (regtr_maxpool_gather, regtr_radius_query,
 * regtr_kpconv_gather, regtr_instnorm_apply, regtr_mha_fwd, regtr_gemm_x3): a binding generated from another version of the header
 * would pass shifted arguments, so every binding must compare regtr_abi_version() with the REGTR_ABI_VERSION it was written against
 * before its first call (regtr_amd/_lib.py does).  Bumped on any signature change; a new entry point shifts nobody's
 * arguments and does not bump it (the training-augmentation entry points, 3DMatch's and ModelNet's, were added at version 11). */
#define REGTR_ABI_VERSION 11
int regtr_abi_version(void);

/* The STATUS WORD: an optional device int (zeroed by the caller, e.g. once per forward) that kernels OR bits into -- conditions that
 * only the data can reveal, reported without a host round trip per launch.  `status` arguments may be NULL.
 *   REGTR_STATUS_F16_RANGE       an f16 pair product (regtr_gemm_x3 with n_planes = 4, regtr_mha_fwd precision 3) came out non-finite:
 *                                an operand reached f16's range (|x| >= 65504).  The caller re-runs in the bf16x3 format (n_planes 3 /
 *                                precision 0), which has float32's range; regtr_amd.RegTR.forward does, once per forward.
 *   REGTR_STATUS_NONFINITE_POSE  regtr_weighted_procrustes wrote a non-finite R|t (whatever the cause upstream). */
#define REGTR_STATUS_F16_RANGE 1
#define REGTR_STATUS_NONFINITE_POSE 2

/* ---- preprocessing ---------------------------------------------------------------------------------------- */

size_t regtr_grid_subsample_ws_bytes(int n_cap, int n_clouds);

/* Voxel-grid barycentres of every cloud.  xyz [n_cap,3] (live rows: seg_off[n_clouds]); out_xyz [n_cap,3] receives
 * M <= n rows, clouds stacked in order, voxels of a cloud in order of first appearance in the input;
 * out_seg_off [n_clouds+1].  Barycentres are bit-identical to the reference's (float32 sums in input order). */
int regtr_grid_subsample(const float* xyz, const int* seg_off, int n_clouds, int n_cap, float dl, float* out_xyz,
                         int* out_seg_off, void* ws, size_t ws_bytes, void* stream);

/* The same with a choice of output row order: row_order 0 = first appearance (above); 1 = the reference's own order, i.e.
 * the iteration order of the libstdc++ std::unordered_map<size_t, .> it fills in input order (grid_subsampling.cpp:48,58-59,85)
 * -- the parity mode (cfg.kpconv_ref_row_order); one thread per cloud replays the container (csrc/ref_umap.h). */
size_t regtr_grid_subsample_ordered_ws_bytes(int n_cap, int n_clouds, int row_order);
/* key_mode: which of the reference's two voxel rules.
 *   0  floor((p - origin) / dl), origin = floor(min corner * (1 / dl)) * dl, linear size_t key -- the CPU Preprocessor's
 *      cpp_subsampling (grid_subsampling.cpp:25-31,53-56); bit-exact against the unmodified reference C++;
 *   1  floor(p / dl), no origin shift, float32 IEEE division -- PreprocessorGPU, the class the reference model instantiates
 *      (regtr.py:29; kpconv.py:213-240: MinkowskiEngine quantisation of points / sampleDl);
 *   2  floor(p * (1 / dl)), reciprocal rounded to float32 -- the same rule as torch's CUDA division by a host scalar evaluates it.
 * 0 and 1 give DIFFERENT voxel sets wherever points sit on voxel faces (3DMatch fragments lie on a lattice: red-kitchen pair
 * 9 977 vs 10 088 level-1 points).  Barycentre arithmetic and the first-appearance row order are the same for every mode
 * (MinkowskiEngine's own output order and summation order are unspecified).  row_order 1 requires key_mode 0.
 * out_cap: rows of out_xyz (<= 0 or > n_cap: n_cap).  The output size is data dependent and only known on the device; a caller that
 * allocates less than n_cap rows gets the first out_cap voxels (first-appearance order), out_seg_off SATURATED at out_cap, and detects
 * the full level by out_seg_off[n_clouds] == out_cap (then repeats with a larger capacity).  row_order 1 needs out_cap = n_cap. */
int regtr_grid_subsample_ordered(const float* xyz, const int* seg_off, int n_clouds, int n_cap, float dl, int row_order, int key_mode,
                                 int out_cap, float* out_xyz, int* out_seg_off, void* ws, size_t ws_bytes, void* stream);

size_t regtr_cellgrid_ws_bytes(int ns_cap, int n_clouds);

/* Builds the support-point cell grid for `radius` into ws (kept by the caller, reused by any number of queries). */
int regtr_cellgrid_build(const float* s_xyz, const int* s_seg_off, int n_clouds, int ns_cap, float radius, void* ws,
                         size_t ws_bytes, void* stream);

/* Fixed-radius neighbours within the same cloud, strict d2 < r2 in the reference's float32 arithmetic, rows padded with
 * Ns_total = s_seg_off[n_clouds].  out_idx [nq_cap,K]:
 *   order 0  the K NEAREST supports in the ball, ascending (d2, support index) -- the reference's CPU Preprocessor
 *            (nanoflann radius search + sort, kpconv.py:243-258; cpp_neighbors/neighbors.cpp:211-332);
 *   order 1  the FIRST K supports in the ball by support index, ascending by index -- the reference's PreprocessorGPU
 *            (pytorch3d ball_query, kpconv.py:261-288), the class its model instantiates (regtr.py:29).
 * The two differ only on rows whose ball holds more than K supports.  out_count [nq_cap] (optional):
 * untruncated in-ball count; out_max_count (optional, device int zeroed by the caller): max over out_count, i.e. the
 * row width the reference's batch_query would return.  1 <= K <= 448.  ns_cap / ws_bytes as given to the build. */
int regtr_radius_query(const float* q_xyz, const int* q_seg_off, int nq_cap, const int* s_seg_off, int ns_cap,
                       int n_clouds, float radius, int K, int order, const void* grid_ws, size_t ws_bytes, int* out_idx,
                       int* out_count, int* out_max_count, void* stream);

/* The same table for the grid's OWN supports as queries (every conv table of the pyramid): a cell-centric kernel -- one wave
 * per occupied cell stages the 27 neighbouring runs once in LDS and answers all of the cell's queries from there.  out_idx
 * [ns_cap, K] is indexed by the original support row; results are identical to regtr_radius_query(s_xyz, s_seg_off, ...). */
int regtr_radius_query_self(const int* s_seg_off, int ns_cap, int n_clouds, float radius, int K, int order, const void* grid_ws,
                            size_t ws_bytes, int* out_idx, int* out_count, int* out_max_count, void* stream);

/* ---- ground-truth overlap (training / validation side) ------------------------------------------- */

/* utils/pointcloud.py:8-65 compute_overlap: index of the NEAREST support of the query's cloud with d2 < radius^2, distances
 * in float64 like open3d's KDTreeFlann (float32 coordinates widened), -1 when the ball is empty.  Query cloud c searches
 * support cloud c (stack src clouds as supports and tgt clouds as queries, then the other way round).  grid_ws: a cell grid
 * built by regtr_cellgrid_build over the supports with grid_radius * (1 + 1e-6) >= radius.  out_idx [nq_cap]. */
int regtr_nearest_in_radius(const float* q_xyz, const int* q_seg_off, int nq_cap, const int* s_seg_off, int ns_cap,
                            int n_clouds, double radius, float grid_radius, const void* grid_ws, size_t ws_bytes, int* out_idx,
                            void* stream);

/* models/backbone_kpconv/kpconv.py:553-562 compute_overlaps, one pyramid level: out[q] = clamp(mean of ov over the valid
 * (0 <= i < ns) entries of the first H columns of row q of nbr, 0, 1); a row without a valid entry gives NaN as in the reference.
 * The library's own tables pad with ns; a negative entry of a caller's table counts as padding too (it is never used as an index). */
int regtr_overlap_avgpool(const float* ov, int ns, const int* nbr, int ld_nbr, int nq, int H, float* out, void* stream);

/* (Parity mode's neighbour tables in the reference's KD-tree / std::sort row order: include/regtr_hip_parity.h, libregtr_parity.so --
 * since ABI 11 a library of its own, so that the product library holds no nanoflann-derived code.) */

/* ---- KPConv encoder --------------------------------------------------------------------------------------- */

/* flag[j] = (sum_c x'[j,c] > 0) ? 1 : 0   -- the per-support term of the reference's normaliser (kpconv_blocks.py:409-410).
 * x' = x, or LeakyReLU_slope(InstanceNorm(x)) when stats [n_seg,C,2] + seg_off [n_seg+1] are given (fused UnaryBlock tail). */
int regtr_rowsum_positive(const float* x, int n, int C, const float* stats, const int* seg_off, int n_seg, float slope,
                          float* flag, void* stream);

/* 1 when regtr_kpconv_gather derives the positivity flags from the feature rows it gathers anyway (Cin == 1 or a
 * multiple of 32 with H <= 64, 16-byte aligned x / wf / x_stats): `flag` may then be NULL and regtr_rowsum_positive skipped. */
int regtr_kpconv_gather_computes_flag(int Cin, int H);

/* wf [nq, KP*Cin] (kernel point major, channel minor), num [nq] = max(1, #positive neighbours).  nbr [nq,H] int32,
 * x [ns,Cin], flag [ns] (or NULL, see above), kernel_points [KP,3], KP <= 16.  x_stats [n_seg,Cin,2] + q_seg_off [n_seg+1] (optional): the
 * gathered features are LeakyReLU_slope(InstanceNorm(x)) computed on the fly (cloud of a neighbour = cloud of its query).
 * s_xyzf (optional, 16-byte aligned [ns,4], no x_stats): per-support records (x, y, z, f) read with ONE 16-byte load per neighbour
 * instead of four scattered 4-byte ones -- the gathers are bound by the texture-address path (TA ~76 % busy, 40 % of its lines were
 * these dwords).  f = the positivity flag (regtr_instnorm_apply writes the records: x is then final, no fold, no row sums); for
 * Cin == 1, f = the feature itself.  ld_wf: row stride of wf in floats, 0 = KP*Cin; only Cin == 1 takes another value (16: rows padded
 * with zeros, the A operand of regtr_block_tail's first-block form). */
int regtr_kpconv_gather(const float* q_xyz, int nq, const float* s_xyz, int ns, const int* nbr, int H, const float* x,
                        int Cin, const float* flag, const float* s_xyzf, const float* kernel_points, int KP, float extent,
                        const float* x_stats, const int* q_seg_off, int n_seg, float slope, float* wf, int ld_wf, float* num,
                        void* stream);

/* out[q,:] = max over the first H columns of row q of nbr (row stride ld_nbr >= H) of x[nbr[q,h],:], the shadow index
 * ns standing for a zero row (kpconv_blocks.py:127-143).  H < ld_nbr serves the reference's CPU tables, whose width is
 * min(max in-ball count, neighborhood_limit) (kpconv.py:255-258): a full row then holds no shadow and its maximum may be negative. */
int regtr_maxpool_gather(const float* x, int ns, int C, const int* nbr, int ld_nbr, int nq, int H, float* out, void* stream);

size_t regtr_instnorm_ws_bytes(int n_clouds, int max_len, int C);
int regtr_instnorm_stats(const float* x, const int* seg_off, int n_clouds, int max_len, int C, float eps, float* stats,
                         void* ws, size_t ws_bytes, void* stream);
/* y = act((x-mean)*rstd [+ residual | + (residual-rmean)*rrstd]); act: 0 none, 1 LeakyReLU(slope); y may alias x.
 * row_positive (optional, C <= 256): [rows] 1.0 where sum_c y[row,c] > 0 -- KPConv's per-support normaliser flag
 * (kpconv_blocks.py:409-410), ready for regtr_kpconv_gather's `flag`; with row_xyz [rows,3] it is written as 16-byte records
 * [rows,4] = (x, y, z, flag) instead: regtr_kpconv_gather's `s_xyzf`. */
int regtr_instnorm_apply(const float* x, const int* seg_off, int n_clouds, int max_len, int C, const float* stats,
                         const float* residual, const float* res_stats, int act, float slope, float* y, const float* row_xyz,
                         float* row_positive, void* stream);

/* ---- dense ------------------------------------------------------------------------------------------------- */

/* C[M,N] = act(A'[M,K] B[K,N] / row_div[m] + bias[n]) + residual[m,n] ; float32 MFMA ; act: 0 none, 1 ReLU.
 * A' = A, or LeakyReLU_slope(InstanceNorm(A)) when a_stats [n_seg,K,2] + a_seg_off [n_seg+1] are given.
 * ws: regtr_gemm_f32_ws_bytes(M,N,K) bytes of scratch for the split-K path (0 for most shapes; ws may then be NULL). */
size_t regtr_gemm_f32_ws_bytes(int M, int N, int K);
int regtr_gemm_f32(const float* A, int lda, const float* B, int ldb, float* C, int ldc, int M, int N, int K,
                   const float* bias, const float* row_div, const float* residual, int ldr, int act,
                   const float* a_stats, const int* a_seg_off, int n_seg, float a_slope, void* ws, size_t ws_bytes,
                   void* stream);

/* The same contraction at float32 accuracy on the bf16 matrix cores (16x the f32-MFMA rate on gfx950): every float32 is
 * split exactly into three bf16 (x = x0 + x1 + x2) and the product is evaluated as six bf16 MFMAs with f32 accumulation;
 * the dropped cross terms are below one f32 ulp of each product.  Weights are split once:
 *   regtr_gemm_split_weights(W, ld, N, K, transposed, planes)   W = [N,K] (nn.Linear.weight as stored; transposed = 0) or
 *                                                               [K,N] (transposed = 1); planes: .._bytes(N, K) bytes
 * regtr_gemm_x3 then has the contract of regtr_gemm_f32 with `planes` in place of B.  Shapes it does not take
 * (regtr_gemm_x3_supported == 0: N not a multiple of 64, K not a multiple of 4) go to regtr_gemm_f32. */
int regtr_gemm_x3_supported(int M, int N, int K);
int regtr_gemm_x3_preferred(int M, int N, int K);   /* supported AND measured faster than regtr_gemm_f32 (K >= 32) */
size_t regtr_gemm_split_weights_bytes(int N, int K);
int regtr_gemm_split_weights(const float* W, int ld, int N, int K, int transposed, void* planes, void* stream);
/* The f16 pair operand format (n_planes = 4 of regtr_gemm_x3): x = h0 + h1 / 2048, h0 = f16(x), h1 = f16((x - h0) * 2048) -- 22 mantissa
 * bits in two planes; a product is three v_mfma_f32_32x32x16_f16 (the two low terms in a second, scaled accumulator) at float32-grade
 * accuracy (error vs float64 within 3x of the six-term bf16 split's on RegTR's shapes), half the matrix-pipe work of the bf16 split.
 * Operands must stay below 65504 in magnitude.  regtr_gemm_x3_f16_supported(M, N, K, with_stats): every shape regtr_gemm_x3 supports. */
int regtr_gemm_x3_f16_supported(int M, int N, int K, int with_stats);      /* with_stats: the call passes stat_partial, a_stats or tile_info
                                                                             * (the launch then keeps regtr_gemm_x3_tile_rows' tile height) */
size_t regtr_gemm_split_weights_f16_bytes(int N, int K);
int regtr_gemm_split_weights_f16(const float* W, int ld, int N, int K, int transposed, void* planes, void* stream);
size_t regtr_gemm_x3_ws_bytes(int M, int N, int K);
int regtr_gemm_x3(const float* A, int lda, const void* planes, float* C, int ldc, int M, int N, int K,
                  const float* bias, const float* row_div, const float* residual, int ldr, int act,
                  const float* a_stats, const int* a_seg_off, int n_seg, float a_slope, void* ws, size_t ws_bytes,
                  double* stat_partial, const int* stat_seg_off, int n_stat_seg, int n_planes, const void* tile_info, int* status,
                  void* stream);
/* status (optional): the status word above; n_planes = 4 reports REGTR_STATUS_F16_RANGE.
 * tile_info (optional): regtr_tile_segments(seg_off, n_seg, M, regtr_gemm_x3_tile_rows(M,N,K), ..) -- 16 bytes per row tile that
 * replace the per-workgroup cloud search (a chain of dependent memory round trips) when a_stats / stat_partial are used; a_seg_off
 * and stat_seg_off must then be the same array. */
int regtr_tile_segments(const int* seg_off, int n_seg, int M, int rows, void* out, void* stream);
int regtr_gemm_x3_tile_rows(int M, int N, int K);
/* n_planes: 3 = the float32-grade six-term product (default everywhere); 2 = three leading terms (a0 w0 + a0 w1 + a1 w0,
 * ~2^-16 relative per product); 1 = plain bf16 operands with float32 accumulation (cfg.compute_dtype 'bf16').  1 and 2 do not
 * combine with a_stats / stat_partial (the KPConv encoder always runs float32-grade). */
/* One-shot strip variant for the shallow encoder levels (K in {32, 64, 128}, N <= 512, millions of rows; csrc/gemm_stream.hip):
 * every wave takes 32 rows from global memory straight into MFMA fragments, the weight planes sit in LDS per 256-row workgroup,
 * nothing is loaded after a store.  Same float32-grade product as regtr_gemm_x3:  C = A' W.
 *   a_stats [n_seg,K,2] (K <= 64): A' = LeakyReLU_a_slope(InstanceNorm(A)); seg_off [n_seg+1]: cloud offsets of the rows;
 *   tile_info = regtr_tile_segments(seg_off, n_seg, M, regtr_gemm_stream_tile_rows(), ..);
 *   stat_partial (optional) = (ceil(M / 256) + n_seg) * N double2 of per-(tile, cloud) column sums of C for
 *   regtr_instnorm_finalize_tiles(tile_rows = 256). */
int regtr_gemm_stream_supported(int M, int N, int K);
int regtr_gemm_stream_tile_rows(void);
int regtr_gemm_stream(const float* A, int lda, const void* planes, float* C, int ldc, int M, int N, int K,
                      const float* a_stats, float a_slope, const int* seg_off, int n_seg, const void* tile_info,
                      double* stat_partial, void* stream);
/* The same call with its launch form named (tests and tools/stream_bench.py; regtr_gemm_stream is form 0): 0 the measured choice per
 * (K, N); 1 one workgroup per (256-row tile, column block); 2 one workgroup per 256-row tile that loads and splits its rows once and walks
 * all column blocks (taken wherever there are two or more).  C and stat_partial hold the same bits in every form.  A new entry point
 * only: no existing signature changes, REGTR_ABI_VERSION stays as it is. */
int regtr_gemm_stream_form(const float* A, int lda, const void* planes, float* C, int ldc, int M, int N, int K,
                           const float* a_stats, float a_slope, const int* seg_off, int n_seg, const void* tile_info,
                           double* stat_partial, int form, void* stream);
int regtr_gemm_stream_walks_columns(int N, int K, int form);   /* 1: that form launches the column-walking kernel for (N, K); host only */
/* Linear -> InstanceNorm [+ Linear -> InstanceNorm of a second input] -> LeakyReLU in one pass over the NARROW inputs
 * (csrc/block_tail.hip):  Y = LeakyReLU_slope( InstanceNorm(A1' W1) [+ InstanceNorm(A2 W2)] ).  The per-cloud statistics of a product
 * come from the K x K second moments of its input (float64), so no product is ever written.  Two served forms
 * (regtr_block_tail_supported):
 *   K1 = 32, K2 = 64, N = 128: the tail of the level-0 resnet block (kpconv_blocks.py:727-741) -- replaces unary2 GEMM + shortcut
 *     GEMM + regtr_instnorm_apply; A1' = LeakyReLU_a1_slope(InstanceNorm(A1)) by a1_stats [n_clouds,K1,2] (the conv output's);
 *   K1 = 16, K2 = 0, N = 64: the first block (:590-646), A1 = the Cin = 1 gather's WF rows at ld_wf = 16, A1' = A1 / row_div1[row]
 *     (the neighbour count, :411), a1_stats / A2 / W2 NULL -- replaces contraction GEMM + statistics + regtr_instnorm_apply.
 * W1 [K1,N] / W2 [K2,N] float32 row-major, seg_off [n_clouds+1], max_len = longest cloud, tile_info = regtr_tile_segments(seg_off,
 * n_clouds, M, 256, ..).  out_stats (optional) [1 or 2,n_clouds,N,2] receives the (mean, rstd) of the products; an empty cloud gets
 * (0, 0), as regtr_instnorm_stats reports it (M = 0 or max_len = 0 launches nothing and writes nothing). */
int regtr_block_tail_supported(int M, int N, int K1, int K2);
size_t regtr_block_tail_ws_bytes(int n_clouds, int max_len, int N, int K1, int K2);
int regtr_block_tail(const float* A1, int lda1, const float* a1_stats, float a1_slope, const float* row_div1, const float* A2, int lda2,
                     const float* W1, const float* W2, const int* seg_off, int n_clouds, int max_len, const void* tile_info,
                     int M, int N, int K1, int K2, float eps, float slope, float* Y, int ldy, void* ws, size_t ws_bytes,
                     float* out_stats, void* stream);

/* InstanceNorm statistics of C straight from the GEMM epilogue (no second pass over C): when
 * R = regtr_gemm_x3_stat_tile_rows(M,N,K) > 0, pass stat_partial = (ceil(M/R) + n_stat_seg) * N * 2 doubles and the cloud
 * offsets of C's rows; then regtr_instnorm_finalize_tiles(stat_partial, seg_off, n_clouds, N, R, eps, stats) yields the
 * same [n_clouds, N, 2] (mean, rstd) table as regtr_instnorm_stats(C).  R = 0 (split-K shapes): not available. */
int regtr_gemm_x3_stat_tile_rows(int M, int N, int K);
int regtr_instnorm_finalize_tiles(const double* partial, const int* seg_off, int n_clouds, int C, int tile_rows, float eps,
                                  float* stats, void* stream);

/* out = a + b over n floats (16-byte aligned pointers): with_pos_embed of the post-norm layer, transformers.py:118-119 */
int regtr_add_f32(const float* a, const float* b, size_t n, float* out, void* stream);

/* y = LayerNorm(x) gamma + beta (+ add); y_plain (optional) the value before add.  Refused (REGTR_ERR_ARG, nothing launched): D < 4,
 * D % 4 != 0, n < 0, a NULL x / gamma / beta / y, a non-null pointer that is not 16-byte aligned (every access is a float4). */
int regtr_layernorm(const float* x, int n, int D, const float* gamma, const float* beta, float eps, const float* add,
                    float* y, float* y_plain, void* stream);

int regtr_posemb_sine(const float* xyz, int n, int npf, int d_model, float scale, const float* dim_t, float* pe,
                      void* stream);

/* pe [n, d_model] = L5(relu(L4(relu(L3(relu(L2(relu(L1(xyz))))))))), the learned positional embedding's five-Linear ReLU MLP
 * 3 -> 32 -> 64 -> 128 -> 256 -> d_model, in one launch: a workgroup owns 32 rows and keeps the hidden activations in LDS.  xyz [n, 3]
 * (12-byte rows, 4-byte aligned).  w_kn / bias: HOST arrays of the five layers' DEVICE pointers, the weights transposed to (K, N) layout:
 * (3, 32), (32, 64), (64, 128), (128, 256), (256, d_model).  acts (optional) [n, 480] = h1 | h2 | h3 | h4, the activations after their
 * ReLUs (what the backward reads); pe does not depend on it being asked for.  Float32 throughout with float32's operand range: L1 on
 * vector FMAs, the others on the exact-f32 MFMA, per element one fmaf chain in k order from zero, + bias, ReLU (v < 0 ? 0 : v: a NaN
 * stays a NaN) -- a row's result is a function of that row and the weights only.  No atomics, no workspace, bit-reproducible.  Rows >= n
 * of pe / acts are not written.  n = 0: REGTR_OK, nothing launched.  Refused (REGTR_ERR_ARG, nothing read or launched): n < 0, d_model
 * not a multiple of 64 in [64, 512], w_kn / bias or one of their entries NULL, xyz or pe NULL with n > 0, a weight / bias / pe / acts
 * pointer that is not 16-byte aligned, xyz not 4-byte aligned. */
int regtr_posemb_mlp(const float* xyz, int n, const float* const* w_kn, const float* const* bias, int d_model, float* pe, float* acts,
                     void* stream);

/* ---- attention + pose -------------------------------------------------------------------------------------- */

/* softmax(q k^T * scale) v per head on packed clouds: cloud c's rows attend the rows of cloud kv_of[c]; head_dim = 32.
 * precision: 0 = float32-grade on the bf16 matrix cores (every operand split exactly into three bf16, six MFMAs per product),
 * 1 = plain bf16 operands with float32 softmax / accumulation (cfg.compute_dtype 'bf16'), 2 = exact-f32 MFMA, 3 = float32-grade by the
 * f16 pair split (x = h0 + h1 / 2048: two planes, three MFMAs per product, a scaled second accumulator; operands below 65504 --
 * q, k, v are projections of LayerNorm outputs, the probabilities are <= 1; what cfg.compute_dtype 'fp32' uses). */
int regtr_mha_fwd(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, float* out, int ldo,
                  const int* seg_off, const int* kv_of, int n_clouds, int max_len, int n_heads, int head_dim, float scale,
                  int precision, int* status, void* stream);      /* status: optional status word (precision 3 reports REGTR_STATUS_F16_RANGE) */

/* The whole pre-norm cross-encoder stack (transformers.py:183-244 forward_pre for every layer, :37-59 the final norm of every
 * layer's output) enqueued by one call -- the same launches, in the same order, as calling regtr_layernorm / regtr_gemm_x3 /
 * regtr_mha_fwd layer by layer (12 per layer); it exists because at one pair per forward the host, not the GPU, is the bound.
 *   x [n_tok, d_model] packed tokens (left untouched)  ->  outs [n_layers | 1, n_tok, d_model]
 *   layer_params  HOST array of n_layers * regtr_cross_encoder_per_layer_params() DEVICE pointers, per layer:
 *                 norm1 gamma, beta | self_attn in_proj planes, bias | out_proj planes, bias | norm2 gamma, beta |
 *                 multihead_attn in_proj planes, bias | out_proj planes, bias | norm3 gamma, beta | linear1 planes, bias |
 *                 linear2 planes, bias          (planes = regtr_gemm_split_weights of the nn.Linear weight)
 *   layer_eps     HOST array, 3 floats per layer;  final_gamma NULL = no final LayerNorm (plain copy)
 *   pe            [n_tok, d_model] added to the normalised tokens for q, k and v (sa/ca_val_has_pos_emb = true), or NULL
 *   supported():  head_dim 32 and every Linear on the split kernel; otherwise issue the launches one by one.
 *   ws            regtr_cross_encoder_ws_bytes(n_tok, d_model, d_ff) bytes */
int regtr_cross_encoder_per_layer_params(void);
int regtr_cross_encoder_supported(int n_tok, int d_model, int d_ff, int n_heads);
size_t regtr_cross_encoder_ws_bytes(int n_tok, int d_model, int d_ff);
int regtr_cross_encoder_fwd(const float* x, int n_tok, int d_model, int d_ff, int n_heads, int n_layers,
                            const void* const* layer_params, const float* layer_eps, const float* final_gamma,
                            const float* final_beta, float final_eps, int return_intermediate, const float* pe,
                            const int* seg_off, const int* kv_self, const int* kv_cross, int n_clouds, int max_len,
                            int gemm_planes, int attn_precision, void* ws, size_t ws_bytes, float* outs, int* status, void* stream);

/* The KPConv encoder's blocks (kpconv.py:81-88 KPFEncoder.forward over kpconv_blocks.py:632-646 SimpleBlock.forward and :706-741
 * ResnetBottleneckBlock.forward) enqueued by ONE call, for the SMALL-batch regime: a pair or two per forward -- the reference's own
 * operating mode (conf/3dmatch.yaml:11 test_batch_size 1, trainer.py:202-206), where the host, not the GPU, bounds an op-by-op forward.
 * The same launches, with the same arguments, in the same order as regtr_amd/kpconv.py issues them through the entry points above
 * (outputs bit-identical); intermediates carved from one workspace.  HOST-side descriptors: */
typedef struct {
    const float* kn;        /* [K, N] float32 row-major (regtr_gemm_f32's B) */
    const void* planes;     /* regtr_gemm_split_weights of the matrix, or NULL (shape not served by regtr_gemm_x3) */
    const void* planes16;   /* regtr_gemm_split_weights_f16, or NULL (a weight beyond the f16 range: stays on `planes`) */
    int N, K;               /* N == 0: no such Linear in the block (identity) */
} regtr_weight_t;
typedef struct {
    int kind;               /* 0 SimpleBlock, 1 ResnetBottleneckBlock */
    int strided;            /* 1: the convolution reads level `layer` and writes level `layer + 1` (pool table, max-pooled shortcut) */
    int layer;
    int n_kp;               /* kernel points (<= 16) */
    float extent;           /* KP_extent of the block's KPConv */
    const float* kernel_points;     /* [n_kp, 3] */
    regtr_weight_t unary1;  /* kind 1: Linear in front of the KPConv (N == 0: nn.Identity) */
    regtr_weight_t conv;    /* KPConv.weights viewed as [n_kp * Cin, Cout] */
    regtr_weight_t unary2;  /* kind 1 */
    regtr_weight_t shortcut;        /* kind 1: unary_shortcut (N == 0: nn.Identity) */
} regtr_encoder_block_t;
typedef struct {
    const float* points;    /* [n, 3] */
    int n;                  /* live rows of the level (host-known: the one read-back of a forward) */
    const int* conv_idx;    /* [n, K] neighbour table of the level, or NULL */
    const int* pool_idx;    /* [n of the NEXT level, K] supports of this level per next-level point, or NULL */
    int K;                  /* columns of both tables */
    int pool_width;         /* columns of pool_idx the strided shortcut's max-pool reads (K; the parity mode's narrower CPU tables) */
    const int* seg_off;     /* [n_clouds + 1] */
    int max_len;            /* longest cloud of the level */
} regtr_encoder_level_t;
/* supported(): the shapes; the CALLER keeps the call to its small-batch regime (regtr_amd/ops.py SMALL_REGIME_ROWS = 131072 level-0 rows:
 * below it no large-batch kernel form applies -- which is the routing this function implements); otherwise issue the launches one by one.  x_in [rows of block `first`'s level, its input width] -> out [rows of block `last - 1`'s level, its width];
 * blocks [first, last).  f16_pair: contractions in the f16 pair format where planes16 exists and the kernel serves the shape (what
 * cfg.compute_dtype 'fp32' runs); ws: regtr_encoder_ws_bytes(...) bytes for the same arguments. */
int regtr_encoder_supported(const regtr_encoder_block_t* blocks, int n_blocks, const regtr_encoder_level_t* levels, int n_levels,
                            int n_clouds, int first, int last);
size_t regtr_encoder_ws_bytes(const regtr_encoder_block_t* blocks, int n_blocks, const regtr_encoder_level_t* levels, int n_levels,
                              int n_clouds, int first, int last, int f16_pair);
int regtr_encoder_fwd(const regtr_encoder_block_t* blocks, int n_blocks, const regtr_encoder_level_t* levels, int n_levels, int n_clouds,
                      int first, int last, const float* x_in, float* out, int f16_pair, float slope, float eps, void* ws, size_t ws_bytes,
                      int* status, void* stream);

/* CorrespondenceDecoder.simple_attention (regtr.py:316-351, `direct_regress_coor: False`): single-head attention whose values
 * are coordinates.  q, k [n_layers, n_total, head_dim] contiguous (projections of the conditioned features), xyz [n_total,3],
 * out [n_layers, n_total, 3]; cloud c attends cloud kv_of[c]; head_dim in {32, 64, 128, 256}. */
int regtr_attn_xyz(const float* q, const float* k, const float* xyz, float* out, const int* seg_off, const int* kv_of,
                   int n_clouds, int n_total, int n_layers, int max_len, int head_dim, float scale, void* stream);

/* kp [n_total,3], corr [L,n_total,3], logit [L,n_total], seg_off [2*n_pairs+1] -> pose [L,n_pairs,3,4]; status (optional): the
 * status word, REGTR_STATUS_NONFINITE_POSE when an R|t came out non-finite */
int regtr_weighted_procrustes(const float* kp, const float* corr, const float* logit, const int* seg_off, int n_pairs,
                              int n_total, int n_layers, float* pose, int* status, void* stream);

/* The backward of regtr_weighted_procrustes in closed form (no SVD derivative; csrc/procrustes.hip states it): the same inputs and
 * d_pose [L,n_pairs,3,4], the gradient of every R|t -> d_corr [L,n_total,3]; optionally (NULL: not written) d_logit [L,n_total],
 * d_kp [L,n_total,3] -- PER LAYER, kp's gradient is their sum over L -- and d_weight [L,n_total], the gradient with respect to
 * w = sigmoid(logit) (d_logit without the factor w (1 - w), finite at w = 0 and 1).  One workgroup per (pair, layer) recomputes the
 * forward with the forward's own code, nothing is saved by the forward; float64 fixed-tree sums, every row written once by one thread:
 * no atomics, no workspace, bit-reproducible, no host wait.  A pair whose R is no differentiable function of its float32 inputs gets
 * exactly zero rows: min_{i<j} (lam_i + lam_j) <= 2^-23 lam_0 with lam = (S0, S1, d S2) (the zero covariance, collinear points, a
 * reflection with S1 = S2), a weight sum at the 1e-6 clamp, an empty pair.  The other pairs of the launch are unaffected. */
int regtr_weighted_procrustes_bwd(const float* kp, const float* corr, const float* logit, const int* seg_off, int n_pairs, int n_total,
                                  int n_layers, const float* d_pose, float* d_corr, float* d_logit, float* d_kp, float* d_weight,
                                  void* stream);


/* ---- validation / test losses (models/regtr.py:237-294 compute_loss; inference only, no gradients) ----------------------------- */

/* InfoNCE feature loss (models/losses/feature_loss.py:246-314) over packed, ragged pairs.  Pair b's anchors are rows
 * [anc_seg_off[b], anc_seg_off[b+1]) of anc [n_anc, D] (row stride ld_anc), its targets rows [pos_seg_off[b], pos_seg_off[b+1]) of
 * pos [n_pos, D] (row stride ld_pos), which hold the TRANSFORMED positives P' = G W_sym.  Per anchor row i, over the pair's targets j:
 *   l_ij = A_i . P'_j (exact f32 MFMA), d_ij = sqrt_rn((dx^2 + dy^2) + dz^2) in float32 without contraction,
 *   j* = argmin_j d_ij -- on exact ties the LOWEST j --, mask_i = d_ij* < r_p, ignore_ij = d_ij < r_n && j != j*,
 *   loss_i = -l_ij* + logsumexp over the j not ignored.
 * anc_pose: NULL, or [n_pairs, 12] row-major 3x4 poses applied to the anchor coordinates first (x' = ((R0 x + R1 y) + R2 z) + t,
 * rounded per operation).  pair_out [n_pairs, 2]: (sum of loss_i over masked rows, number of masked rows) -- reduced in a fixed
 * order, bit-reproducible.  row_loss / row_mask [n_anc]: optional (NULL) per-row loss_i and mask_i (1 / 0); a row of a pair without
 * targets gets NaN / 0.  max_anc >= every pair's anchor count (a pair with more, or with offsets outside the arrays, gives NaN).
 * Refused (REGTR_ERR_ARG, nothing launched): D not a multiple of 64 or above 512, a negative count, a NULL pointer with a non-zero
 * count, ld < D, rows of anc / pos not 16-byte aligned.  ws: regtr_infonce_ws_bytes(n_pairs, max_anc) bytes. */
size_t regtr_infonce_ws_bytes(int n_pairs, int max_anc);
int regtr_infonce(const float* anc, int ld_anc, const float* pos, int ld_pos, const float* anc_xyz, const float* pos_xyz,
                  const int* anc_seg_off, const int* pos_seg_off, int n_pairs, int n_anc, int n_pos, int max_anc, int D,
                  float r_p, float r_n, const float* anc_pose, float* pair_out, float* row_loss, float* row_mask, void* ws,
                  size_t ws_bytes, void* stream);

/* The O(N) loss terms of one decoder layer, per pair b of the packed coarsest-level tokens (seg_off [2 n_pairs + 1]: the src clouds,
 * then the tgt clouds, as RegTR.forward packs them), into out [n_pairs, 5]:
 *   0: sum of BCE-with-logits(logit, gt_overlap) over the pair's src and tgt tokens, max(x,0) - x y + log1p(exp(-|x|)) in float64;
 *   1, 2: sum of w |warped - T kp|_1 and sum of w over the src tokens (T = pose b, w = gt_overlap)   models/losses/corr_loss.py:18-40;
 *   3, 4: the same over the tgt tokens with T^-1 = [R^T | -R^T t].
 * pose: [n_pairs] poses of pose_stride floats (12: 3x4, 16: 4x4), rows 0-2 read.  Transforms and L1 errors in float32 rounded per
 * operation, sums in float64, fixed-order reductions.  Refused like regtr_infonce (negative counts, NULLs with a non-zero count,
 * pose_stride not 12 or 16). */
/* x' = ((R0 x + R1 y) + R2 z) + t, rounded per operation, for every point of packed clouds: point i of cloud c (seg_off[c] <= i <
 * seg_off[c + 1], n_clouds + 1 entries, seg_off[0] = 0, seg_off[n_clouds] = n) takes pose c (pose_stride 12: 3x4, 16: 4x4).  out [n, 3]. */
int regtr_se3_transform(const float* xyz, const int* seg_off, int n_clouds, int n, const float* pose, int pose_stride, float* out,
                        void* stream);

int regtr_loss_terms(const float* logit, const float* gt_overlap, const float* kp, const float* warped, const int* seg_off,
                     int n_pairs, int n_total, const float* pose, int pose_stride, float* out, void* stream);


/* ---- training-loss backward (regtr_amd/losses.py: the InfoNCELossFull / CorrCriterion drop-ins) ------------------------------------ */

/* regtr_infonce with the per-row decisions the backward reuses: besides regtr_infonce's outputs (row_loss may be NULL, row_mask may
 * not), row_lse [n_anc] = the logsumexp over the allowed set and row_idx [n_anc] = j*_i, the packed positive index of the argmin
 * (-1 and NaN when the pair has no targets).  pair_out, row_loss and row_mask are bit-identical to regtr_infonce's.  Refused like
 * regtr_infonce, and when n_anc > 0 with row_mask, row_lse or row_idx NULL. */
int regtr_infonce_rows(const float* anc, int ld_anc, const float* pos, int ld_pos, const float* anc_xyz, const float* pos_xyz,
                       const int* anc_seg_off, const int* pos_seg_off, int n_pairs, int n_anc, int n_pos, int max_anc, int D,
                       float r_p, float r_n, const float* anc_pose, float* pair_out, float* row_loss, float* row_mask, float* row_lse,
                       int* row_idx, void* ws, size_t ws_bytes, void* stream);

/* Backward of regtr_infonce_rows' mean over pairs, loss = (1 / mean_div) sum_b pair_out[b,0] / pair_out[b,1], from the forward's own
 * decisions (row_lse, row_idx, row_mask, pair_out) and the same distance arithmetic / anchor pose.  grad: ONE float on the device (the
 * upstream gradient g); s_b = (g / mean_div) / pair_out[b,1] is formed on the device.  Over the allowed set of masked rows,
 *   dl_ij = s_b exp(l_ij - LSE_i) - s_b [j = j*_i],   d_anc_i = sum_j dl_ij P'_j,   d_pos_j = sum_i dl_ij A_i
 * (d_pos is the gradient of the TRANSFORMED positives P'); unmasked rows and ignored entries contribute 0.  Every row of every pair
 * is written (pairs without columns give 0 rows); rows outside every pair are not.  Exact-f32 MFMA, one owner per output row,
 * bit-reproducible.  max_anc / max_pos >= every pair's anchor / positive count.  Refused like regtr_infonce (and mean_div <= 0,
 * ld_danc / ld_dpos < D). */
int regtr_infonce_bwd(const float* anc, int ld_anc, const float* pos, int ld_pos, const float* anc_xyz, const float* pos_xyz,
                      const int* anc_seg_off, const int* pos_seg_off, int n_pairs, int n_anc, int n_pos, int max_anc, int max_pos,
                      int D, float r_n, const float* anc_pose, const float* row_lse, const int* row_idx, const float* row_mask,
                      const float* pair_out, const float* grad, float mean_div, float* d_anc, int ld_danc, float* d_pos, int ld_dpos,
                      void* stream);

/* out [N1, N2] (row stride ldo) = a^T b for a [M, N1] and b [M, N2] (row strides lda, ldb) over a tall M: exact-f32 MFMA, split-K
 * with a fixed-order float64 second pass, bit-reproducible.  fold = 1 (N1 == N2) writes InfoNCELossFull's dW from dW_sym = a^T b
 * instead: out_ij = dW_sym_ij + dW_sym_ji for i < j, 2 dW_sym_ii on the diagonal, 0 below.  Refused: N1 or N2 not a positive
 * multiple of 64, a negative M, a stride below its width, NULLs.  ws: regtr_gemm_tn_ws_bytes(M, N1, N2) bytes. */
size_t regtr_gemm_tn_ws_bytes(int M, int N1, int N2);
int regtr_gemm_tn(const float* a, int lda, const float* b, int ldb, int M, int N1, int N2, int fold, float* out, int ldo, void* ws,
                  size_t ws_bytes, void* stream);

/* Backward of CorrCriterion('mae') (models/losses/corr_loss.py:24-37): d_warped [n, 3] = ((g / den) w_i) sgn(warped - T kp), sgn(0)
 * = 0, with T kp rounded per operation as regtr_loss_terms rounds it.  Point i of cloud c (seg_off [n_clouds + 1]) takes pose c
 * (pose_stride 12 or 16); grad and den (the clamped weight sum) are ONE float each on the device.  Refused like regtr_se3_transform. */
int regtr_corr_l1_bwd(const float* kp, const float* warped, const float* w, const int* seg_off, int n_clouds, int n, const float* pose,
                      int pose_stride, const float* grad, const float* den, float* d_warped, void* stream);

/* CircleLossFull with dist_type 'euclidean' (models/losses/feature_loss.py:160-243) over packed, ragged pairs: regtr_infonce_rows'
 * argument conventions (anc / pos with row strides, the two segment-offset tables, anc_pose applied to the anchor coordinates on load;
 * pos holds the positives' features themselves), plus max_pos.  Per pair, over anchors i and positives j:
 *   d_ij = sqrt(sum_c (a_ic - b_jc)^2 + 1e-12), the explicit differences accumulated in float32 (c ascending, fused multiply-add);
 *   pos_ij = cd_ij < r_p, neg_ij = cd_ij > r_n with cd_ij regtr_infonce's coordinate distance (the same arithmetic, both strict);
 *   tp_ij = s (d - pos_margin) max(d - pos_optimal, 0) where pos_ij, else 0;  tn_ij = s (neg_margin - d) max(neg_optimal - d, 0) where
 *   neg_ij, else 0 -- a masked entry enters its log-sum-exp as exp(0), as in the reference;
 *   row_i = softplus(LSE_j tp_ij + LSE_j tn_ij) / s, selected when row i has a pos and a neg; col_j the same over i.
 * anc_lse [n_anc, 2] / pos_lse [n_pos, 2]: the two log-sum-exps of every row / column (max-subtracted, online); anc_sel [n_anc] /
 * pos_sel [n_pos]: the selection flags (1 / 0).  pair_out [n_pairs, 4]: (sum of the selected row_i, their number, sum of the selected
 * col_j, their number), float64 sums in a fixed order: no atomics, bit-reproducible; the pair loss is (out0 / out1 + out2 / out3) / 2
 * (NaN for an empty selection).  max_anc / max_pos >= every pair's counts (a pair with more, or with offsets outside the arrays,
 * gives NaN sums).  No workspace.  Refused (REGTR_ERR_ARG, nothing launched): D not a multiple of 64 or above 512, a negative count,
 * a NULL pointer with a non-zero count, ld < D or not a multiple of 4, anc / pos not 16-byte aligned, log_scale <= 0. */
int regtr_circle_rows(const float* anc, int ld_anc, const float* pos, int ld_pos, const float* anc_xyz, const float* pos_xyz,
                      const int* anc_seg_off, const int* pos_seg_off, int n_pairs, int n_anc, int n_pos, int max_anc, int max_pos, int D,
                      float r_p, float r_n, float log_scale, float pos_margin, float pos_optimal, float neg_margin, float neg_optimal,
                      const float* anc_pose, float* pair_out, float* anc_lse, float* anc_sel, float* pos_lse, float* pos_sel,
                      void* stream);

/* Backward of loss = (1 / mean_div) sum_b (out0 / out1 + out2 / out3)_b / 2 from regtr_circle_rows' statistics and the same distance
 * arithmetic.  grad: ONE float on the device.  The weights max(.) are constants of the differentiation, so with
 *   k_i = (grad / mean_div / 2 / out1) sigmoid(LSEp_i + LSEn_i) on selected rows (0 elsewhere), k_j likewise with out3 on columns,
 *   g_ij = (k_i e^(tp - LSEp_i) + k_j e^(tp - LSEp_j)) max(d - pos_optimal, 0) [pos_ij]
 *        - (k_i e^(tn - LSEn_i) + k_j e^(tn - LSEn_j)) max(neg_optimal - d, 0) [neg_ij],      c_ij = g_ij / d_ij,
 *   d_anc_i = (sum_j c_ij) a_i - sum_j c_ij b_j,      d_pos_j = (sum_i c_ij) b_j - sum_i c_ij a_i.
 * Every row of every pair is written; a pair whose loss is NaN (out1 = 0 or out3 = 0) gets zero rows.  One owner per output row, no
 * atomics, no host wait, bit-reproducible.  Refused like regtr_circle_rows, and: mean_div <= 0, ld_danc / ld_dpos < D or not a
 * multiple of 4, d_anc / d_pos not 16-byte aligned. */
int regtr_circle_bwd(const float* anc, int ld_anc, const float* pos, int ld_pos, const float* anc_xyz, const float* pos_xyz,
                     const int* anc_seg_off, const int* pos_seg_off, int n_pairs, int n_anc, int n_pos, int max_anc, int max_pos, int D,
                     float r_p, float r_n, float log_scale, float pos_margin, float pos_optimal, float neg_margin, float neg_optimal,
                     const float* anc_pose, const float* anc_lse, const float* anc_sel, const float* pos_lse, const float* pos_sel,
                     const float* pair_out, const float* grad, float mean_div, float* d_anc, int ld_danc, float* d_pos, int ld_dpos,
                     void* stream);

/* Backward of regtr_mha_fwd's arithmetic on the same packed layout (head_dim = 32; cloud c's rows attend the rows of cloud kv_of[c]; any
 * kv_of with entries in [0, n_clouds) is legal, several query clouds may share a key cloud).  With s_ij = scale q_i . k_j, P = softmax_j(s),
 * dP_ij = d_out_i . v_j and delta_i = sum_j P_ij dP_ij, per head:
 *   dv_j = sum_i P_ij d_out_i,   dS_ij = P_ij (dP_ij - delta_i),   dq_i = scale sum_j dS_ij k_j,   dk_j = scale sum_i dS_ij q_i.
 * A function of (q, k, v, d_out) and the layout only: S and the row statistics are recomputed and the forward's output is not read, so
 * the result is the same whichever forward precision produced it.  Two launches: a query-tile-owner pass writes dq and the per-(head,
 * row) logsumexp and delta (delta from its own online accumulation) into ws; a key-tile-owner pass writes dk and dv, walking the query
 * clouds in ascending order.  Every row of every cloud is written (a cloud nobody attends gets zero dk / dv rows, a cloud attending an
 * empty cloud zero dq rows); rows outside every cloud are not.  Exact-f32 MFMA, float32 softmax statistics, one owner per output row,
 * no atomics, bit-reproducible.  n_total = rows of the packed arrays (>= seg_off[n_clouds]); max_len >= every cloud's length (0:
 * nothing to do, REGTR_OK).  Refused (REGTR_ERR_ARG, nothing launched): a NULL pointer with work to do, n_clouds < 1, a negative
 * count, n_heads < 1, head_dim != 32, an ld that is not a multiple of 4 or is below n_heads * 32, a base pointer not 16-byte aligned.
 * ws: regtr_mha_bwd_ws_bytes(n_total, n_heads) bytes (REGTR_ERR_WORKSPACE when smaller; 0 for a negative count). */
size_t regtr_mha_bwd_ws_bytes(int n_total, int n_heads);
int regtr_mha_bwd(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, const float* d_out, int ld_do,
                  float* dq, int ld_dq, float* dk, int ld_dk, float* dv, int ld_dv, const int* seg_off, const int* kv_of,
                  int n_clouds, int n_total, int max_len, int n_heads, int head_dim, float scale, void* ws, size_t ws_bytes,
                  void* stream);

/* Backward of regtr_layernorm.  x [n, D] the forward's input, dy [n, D] the gradient of its output y (a caller that used y and y_plain
 * passes the sum of their gradients; the gradient of `add` is dy itself), dres [n, D] optional: a gradient that reached x by another
 * branch (the layer's residual), added into dx.  Mean and rstd are recomputed from x in the forward's operation order -- nothing is
 * saved by the forward, and xh = (x - mean) rstd is the value it used.  With g = dy gamma:
 *   dx = rstd (g - mean_c(g) - xh mean_c(g xh)) [+ dres],   dgamma_c = sum_rows dy xh,   dbeta_c = sum_rows dy.
 * Two launches: one wave per row writes dx and adds its rows' dy xh and dy into per-workgroup partials over fixed row chunks (the chunk
 * height depends on n only); a second launch adds the chunks of a column in a fixed order in float64.  One owner per output element, no
 * atomics, bit-reproducible.  dx may be dres (not x or dy).  n = 0: nothing to do, REGTR_OK, nothing written.  Refused (REGTR_ERR_ARG,
 * nothing launched): n < 0, D < 4, D % 4 != 0, D > 1024 (a lane keeps its column sums in registers), a NULL pointer other than dres
 * with work to do, a pointer that is not 16-byte aligned.  ws: regtr_layernorm_bwd_ws_bytes(n, D) bytes (REGTR_ERR_WORKSPACE when
 * smaller; 0 when there is nothing to do or the shape is refused). */
size_t regtr_layernorm_bwd_ws_bytes(int n, int D);
int regtr_layernorm_bwd(const float* x, int n, int D, const float* gamma, float eps, const float* dy, const float* dres, float* dx,
                        float* dgamma, float* dbeta, void* ws, size_t ws_bytes, void* stream);

/* Column sums of a gradient g [n, N] (row stride ldg), optionally through a ReLU mask:
 *   h == NULL:  db_c = sum_rows g                                    (the bias gradient of a Linear whose output gradient is g)
 *   h [n, N]:   dh = g where h > 0, else +0;  db_c = sum_rows dh     (h: what the forward stored AFTER its ReLU; h == 0 takes gradient 0,
 *                                                                     as torch's ReLU backward does).  dh is optional and may be g.
 * Two launches like regtr_layernorm_bwd's: per-workgroup partial sums over fixed row chunks (a function of n only), each thread adding
 * its rows in row order, then the chunks of a column in a fixed order in float64.  One owner per output element, no atomics,
 * bit-reproducible.  n = 0: nothing to do, REGTR_OK, nothing written.  Refused (REGTR_ERR_ARG, nothing launched): n < 0, N < 4,
 * N % 4 != 0, a row stride below N or not a multiple of 4 (ldh / ld_dh are read only when h / dh is given), dh without h, g, db or ws
 * NULL with work to do, a base pointer that is not 16-byte aligned.  ws: regtr_bias_relu_bwd_ws_bytes(n, N) bytes
 * (REGTR_ERR_WORKSPACE when smaller). */
size_t regtr_bias_relu_bwd_ws_bytes(int n, int N);
int regtr_bias_relu_bwd(const float* g, int ldg, const float* h, int ldh, float* dh, int ld_dh, float* db, int n, int N, void* ws,
                        size_t ws_bytes, void* stream);

/* ---- KPConv backward (regtr_amd/kpconv_grad.py: KPConv.forward_grad) ---------------------------------------------------------------- */

/* The neighbour table by SUPPORT.  nbr [nq, H] int32 (rows of queries, entries = support indices, anything outside [0, ns) a shadow)
 * -> a CSR table: row_off [ns + 1] and entries [nq H] (the first row_off[ns] live): support s's incoming entries q H + h with
 * nbr[q, h] == s are entries[row_off[s] .. row_off[s + 1]), in ASCENDING order.  Shadow entries are dropped.  The in-degree of a
 * support is not bounded by H.  Six launches: count (integer atomics, whose sums do not depend on their order), a three-launch
 * exclusive scan, fill through atomic cursors into a scratch list, then one wave per support puts its list in ascending order (rank
 * among the list's distinct entries; lists above 64 entries are ranked against memory, quadratic in the list length) -- so the table
 * is a pure function of nbr, whatever the scheduling.  Nothing about it is KPConv's: a max-pool backward walks the same table.
 * An empty table (nq = 0 or ns = 0) zeroes row_off and launches nothing else (nbr / entries / ws may then be NULL).  Refused
 * (REGTR_ERR_ARG, nothing launched): a negative count, H < 1, nq H >= 2^31, row_off NULL, nbr / entries / ws NULL with work to do.
 * ws: regtr_nbr_transpose_ws_bytes(nq, H, ns) bytes (REGTR_ERR_WORKSPACE when smaller; 0 for a refused shape). */
size_t regtr_nbr_transpose_ws_bytes(int nq, int H, int ns);
int regtr_nbr_transpose(const int* nbr, int nq, int H, int ns, int* row_off, int* entries, void* ws, size_t ws_bytes, void* stream);

/* Backward of regtr_kpconv_gather with respect to the features: from dwf [nq, KP Cin] (the gradient of wf, row stride KP Cin),
 *   dx[s, c] = sum over the entries e = q H + h of support s (row_off / entries of regtr_nbr_transpose(nbr, nq, H, ns)), ascending,
 *              of sum_k infl(q, s, k) dwf[q, k Cin + c],
 * infl = max(0, 1 - |s_xyz[s] - q_xyz[q] - kernel_points[k]| / extent) recomputed with regtr_kpconv_gather's own statements (uncontracted
 * squared distance, hardware square root, precomputed 1 / extent), never stored.  The entry's column h plays no part, so nbr itself is
 * not read.  One wave owns one row of dx: per-lane sums in (entry, k) order, lanes that walk entries side by side (Cin <= 32) combined
 * by a fixed tree; no atomics, bit-reproducible.  A dwf row whose influence is exactly 0 is not read (so a non-finite value there does
 * not propagate, unlike 0 x inf).  Every row of dx [ns, Cin] is written -- a support without entries gets +0 -- and nothing past it.
 * Entries are clamped to [0, nq H): a table of another nbr cannot make a read leave the arrays.  Cin 1 ... 256 (any), KP <= 16,
 * 1 <= H <= 448.  ns = 0: nothing to do, REGTR_OK.  Refused (REGTR_ERR_ARG, nothing launched): other shapes, a negative count,
 * extent <= 0, nq H >= 2^31, s_xyz / kernel_points / row_off / dx NULL with work to do, dwf / q_xyz / entries NULL with nq > 0, dwf or
 * dx not 16-byte aligned. */
int regtr_kpconv_gather_bwd(const float* dwf, const float* q_xyz, int nq, const float* s_xyz, int ns, int H, int Cin,
                            const float* kernel_points, int KP, float extent, const int* row_off, const int* entries, float* dx,
                            void* stream);

/* out[r, c] = x[r, c] / div[r] (IEEE division), r < n, c < N; row strides ldx, ldo >= N.  KPConv's backward through the neighbour count:
 * g = dOut / num (num is an integer count and carries no gradient).  out may be x.  Refused: n < 0, N < 1, a stride below N, NULLs with
 * work to do. */
int regtr_row_div(const float* x, int ldx, const float* div, int n, int N, float* out, int ldo, void* stream);

/* regtr_gemm_tn (no fold) for ANY positive widths: out [N1, N2] = a^T b, a [M, N1], b [M, N2].  The same split-K scheme with guarded
 * tile edges -- exact-f32 MFMA partial sums over fixed row chunks (a function of M, N1, N2 only), added in chunk order in float64:
 * bit-reproducible.  KPConv's weight gradient WF^T g at KP Cin = 480, Cout = 32 and the first block's 15-wide WF.  Refused: M < 0, a
 * width < 1, N1 N2 >= 2^28, a stride below its width, NULLs.  ws: regtr_gemm_tn_any_ws_bytes(M, N1, N2) bytes. */
size_t regtr_gemm_tn_any_ws_bytes(int M, int N1, int N2);
int regtr_gemm_tn_any(const float* a, int lda, const float* b, int ldb, int M, int N1, int N2, float* out, int ldo, void* ws,
                      size_t ws_bytes, void* stream);

/* ---- InstanceNorm and max-pool backward (regtr_amd/backbone_grad.py: instance_norm, max_pool) ----------------------------------------- */

/* Backward of regtr_instnorm_apply taken together with regtr_instnorm_stats, i.e. of
 *   y = act( (x - mean) rstd  [+ res | + (res - rmean) rrstd] ),   act 0 none / 1 LeakyReLU(slope),
 * per cloud segment and channel, (mean, rstd) = stats and (rmean, rrstd) = res_stats being the biased-variance statistics of x and res
 * (so the gradient flows through them too).  x, seg_off, n_clouds, max_len, C, stats, residual, res_stats, act and slope are exactly
 * what the forward took (stats is required here); dy [N, C] is the gradient of y.  With z the activation's argument, recomputed with
 * the forward's own arithmetic so that every element's LeakyReLU side is the forward's, g = dy (z > 0 ? 1 : slope), xh = (x - mean) rstd
 * and means taken over the cloud's rows:
 *   dx   = rstd (g - mean(g) - xh mean(g xh))
 *   dres = g                                       (plain shortcut: res_stats NULL)
 *        = rrstd (g - mean(g) - rh mean(g rh))     (normalised shortcut, rh = (res - rmean) rrstd)
 * dx and dres are optional (NULL: not wanted), at least one is given, dres needs residual.  Three launches in regtr_instnorm_stats'
 * thread mapping and chunking: per-(cloud, chunk, channel) sums of g, g xh and g rh in float64, one wave per (cloud, channel) adding
 * the chunks in a fixed order, then the apply pass (the first two are skipped when only a plain shortcut's dres is wanted).  One owner
 * per output element, no atomics, bit-reproducible.  Every row of every cloud is written and nothing else; an empty cloud does no
 * work; a one-row cloud gets dx = 0 exactly.  max_len >= every cloud's length; max_len = 0: nothing to do, REGTR_OK.  Refused
 * (REGTR_ERR_ARG, nothing launched): n_clouds < 1, max_len < 0, C not a multiple of 4 with C / 4 a power of two <= 256, act not 0 / 1,
 * x / seg_off / stats / dy NULL, dx and dres both NULL, dres or res_stats without residual, a pointer that is not 16-byte aligned, ws
 * NULL when the sums are needed.  ws: regtr_instnorm_bwd_ws_bytes(n_clouds, max_len, C) bytes (REGTR_ERR_WORKSPACE when smaller; 0 for
 * a refused shape). */
size_t regtr_instnorm_bwd_ws_bytes(int n_clouds, int max_len, int C);
int regtr_instnorm_bwd(const float* x, const int* seg_off, int n_clouds, int max_len, int C, const float* stats, const float* residual,
                       const float* res_stats, int act, float slope, const float* dy, float* dx, float* dres, void* ws, size_t ws_bytes,
                       void* stream);

/* The index regtr_maxpool_gather's maximum came from: for x [ns, C], nbr [nq, ld_nbr] and the first H columns of it (the forward's
 * shapes and ld_nbr / H contract), arg [nq, C] int16: arg[q, c] = the column h whose row wins channel c of query q.  The shadow index
 * ns, or anything outside [0, ns), stands for a zero row.  On equal values the LOWEST column wins (torch.max(dim)'s rule, to which
 * autograd sends the whole gradient); arg = -1 when the winner is a shadow row, which has no gradient target.  x is expected finite (a
 * NaN never wins).  Query owner; the feature rows are read from clamped indices.  nq = 0: nothing to do, REGTR_OK; ns = 0: every arg
 * is -1.  Refused (REGTR_ERR_ARG, nothing launched): a negative count, H < 1, H > 32767, ld_nbr < H, C < 4 or not a multiple of 4,
 * NULLs with work to do, x not 16-byte or arg not 8-byte aligned. */
int regtr_maxpool_argmax(const float* x, int ns, int C, const int* nbr, int ld_nbr, int nq, int H, short* arg, void* stream);

/* regtr_maxpool_gather and regtr_maxpool_argmax in ONE pass over the rows (regtr_maxpool_argmax's thread mapping and loads): out [nq, C]
 * bit-equal to regtr_maxpool_gather's for tables whose shadow entries are >= ns (the preprocessor's), arg [nq, C] equal to
 * regtr_maxpool_argmax's.  nq = 0: nothing to do, REGTR_OK; ns = 0: out is all +0 and every arg is -1.  Refused (REGTR_ERR_ARG, nothing
 * launched): regtr_maxpool_argmax's list, and out NULL or not 16-byte aligned. */
int regtr_maxpool_fwd_argmax(const float* x, int ns, int C, const int* nbr, int ld_nbr, int nq, int H, float* out, short* arg, void* stream);

/* Backward of regtr_maxpool_gather: from dy [nq, C] and arg [nq, C] (regtr_maxpool_argmax),
 *   dx[s, c] = sum over the entries e = q H + h of support s (row_off / entries of regtr_nbr_transpose(nbr, nq, H, ns)), ascending,
 *              of (arg[q, c] == h ? dy[q, c] : +0).
 * Support owner: one lane owns a float4 of channels of one dx row and takes its float32 sum SEQUENTIALLY in ascending entry order, so
 * the result is a pure function of (dy, arg, table) that a float32 restatement reproduces bit for bit.  nbr itself is not read; arg is
 * compared, never used as an index; entries are clamped to [0, nq H) and the list bounds to [0, nq H], so a table of another nbr
 * cannot make a read leave the arrays.  The in-degree of a support is unbounded.  Every row of dx [ns, C] is written -- a support
 * without entries gets +0 -- and nothing past it.  ns = 0: nothing to do, REGTR_OK; nq = 0: dx is all +0, REGTR_OK.  Refused
 * (REGTR_ERR_ARG, nothing launched): a negative count, H < 1, H > 32767, C < 4 or not a multiple of 4, nq H >= 2^31, row_off / dx
 * NULL with ns > 0, dy / arg / entries NULL with nq > 0 and ns > 0, dy / dx not 16-byte or arg not 8-byte aligned. */
int regtr_maxpool_gather_bwd(const float* dy, const short* arg, int nq, int H, int C, const int* row_off, const int* entries, int ns,
                             float* dx, void* stream);

/* ---- correspondence head and overlap loss backward (regtr_amd/head_grad.py) ----------------------------------------------------------- */

/* Backward of CorrespondenceRegressor's two narrow outputs, corr = h2 W4^T + b4 [m, 3] and logit = f wc^T + bc [m], in one pass over
 * the rows.  dcorr [m, 3] and dlogit [m] are the outputs' gradients (either may be NULL: its outputs are then written as +0), h2 [m, D]
 * what coor_mlp[2] stored AFTER its ReLU, f [m, D] the head's input, W4 [3, D], wc [D]:
 *   g2 [m, D] = h2 > 0 ? (dcorr_0 W4_0 + dcorr_1 W4_1) + dcorr_2 W4_2 : +0     (the gradient in front of coor_mlp[2]'s ReLU)
 *   r  [m, D] = dlogit wc                                                     (the logit branch's share of df: the `residual` of the dX GEMM)
 *   dW4 [3, D] = dcorr^T h2,  db4 [3] = sum_rows dcorr,  dwc [D] = dlogit^T f,  dbc [1] = sum_rows dlogit,  db2 [D] = sum_rows g2 (optional)
 * Two launches like regtr_bias_relu_bwd's: per-workgroup partial sums over fixed row chunks (a function of m only), each thread adding
 * its rows in row order, then the chunks of a column in a fixed order in float64.  One owner per output element, no atomics,
 * bit-reproducible.  Rows >= m of g2 / r are not written.  m = 0: nothing to do, REGTR_OK, nothing written.  Refused (REGTR_ERR_ARG,
 * nothing launched): m < 0, D < 64 or not a multiple of 64, a NULL pointer other than dcorr / dlogit / db2 with work to do, h2 / f / W4 /
 * wc / g2 / r / ws not 16-byte aligned, g2 or r aliasing each other or an input.  ws: regtr_head_tail_bwd_ws_bytes(m, D) bytes
 * (REGTR_ERR_WORKSPACE when smaller; 0 when there is nothing to do or the shape is refused). */
size_t regtr_head_tail_bwd_ws_bytes(int m, int D);
int regtr_head_tail_bwd(const float* dcorr, const float* dlogit, const float* h2, const float* f, const float* W4, const float* wc, int m,
                        int D, float* g2, float* r, float* dW4, float* db4, float* dwc, float* dbc, float* db2, void* ws, size_t ws_bytes,
                        void* stream);

/* Backward of mean_i BCEWithLogits(logit_i, target_i) over n points: dlogit_i = (grad / n) (sigmoid(logit_i) - target_i), grad ONE
 * float on the device.  The sigmoid is formed from exp(-|logit|) (no overflow, no cancellation for large |logit|).  n = 0: nothing to
 * do.  Refused: n < 0, NULLs with work to do. */
int regtr_bce_logits_bwd(const float* logit, const float* target, const float* grad, int n, float* dlogit, void* stream);

/* ---- training augmentation (regtr_amd/augment.py: RigidPerturb -> Jitter -> ShufflePoints -> RandomSwap on the device) --------------- */

/* Random numbers of the four entries below: Philox4x32-10 with key = (seed & 0xffffffff, seed >> 32) and counter = (index, cloud_or_pair,
 * purpose, step), purpose 0 pair draws / 1 shuffle keys / 2 jitter; a uniform is ((x >> 8) + 0.5) 2^-24 of one output word, a normal one
 * half of a Box-Muller pair (words (x0, x1) and (x2, x3)).  csrc/augment.hip states which word feeds which decision.  Clouds are packed
 * as 2 n_pairs slots: the src clouds of the pairs, then the tgt clouds. */

/* out [n_clouds, 3] = the mean of every packed cloud's rows (xyz [n, 3], seg_off [n_clouds + 1]): float64 sums in a fixed order (one
 * workgroup per cloud, a strided partial per lane, a fixed tree), rounded once to float32; bit-reproducible.  An empty cloud gives 0.
 * Refused: a negative count, NULLs with work to do. */
int regtr_cloud_centroids(const float* xyz, const int* seg_off, int n_clouds, int n, float* out, void* stream);

/* One thread per pair b: the random decisions of RigidPerturb and RandomSwap and what follows from them.
 *   perturb_mode 0 none: P = identity, perturb_source = 0.
 *                1 small: axis uniform on the sphere, angle = N(0,1) perturb_std pi / sqrt(3), Rodrigues; translation N(0,1)^3 perturb_std /
 *                  sqrt(3); then P <- C^-1 P C, C = translate(-centroid) of the perturbed INPUT cloud (centroids [2 n_pairs, 3]).
 *                2 large: zyx Euler angles uniform in (0, 2 pi), zero translation.
 *   perturb_source = u > 0.5 (the src cloud takes P, else the tgt cloud);  swap = (swap argument != 0) and u > 0.5.
 *   pose_out [n_pairs, 3, 4] = pose o P^-1 (source perturbed) or P o pose (target perturbed), then inverted when swapped.
 *   xform [2 n_pairs, 3, 4]: P for the perturbed input cloud slot, the identity for the other;  flags [n_pairs, 2] = perturb_source, swap.
 * P is formed in float64 and rounded once to float32; every composition after that is float32 rounded per operation with sums taken
 * left to right.  pose: pose_stride 12 (3x4) or 16 (4x4) floats per pair, rows 0-2 read.  Refused: a negative count, another
 * pose_stride or perturb_mode, a negative or NaN perturb_std in mode 1, NULLs with work to do (centroids only in mode 1). */
int regtr_augment_draws(const float* pose, int pose_stride, const float* centroids, int n_pairs, unsigned long long seed,
                        unsigned int step, int perturb_mode, float perturb_std, int swap, float* xform, float* pose_out, int* flags,
                        void* stream);

/* keys [n] int64: (cloud_slot << 32) | word x0 of counter (row within the cloud, cloud_slot, 1, step), for every row of the packed
 * clouds (seg_off [n_clouds + 1], seg_off[n_clouds] = n).  Their stable ascending sort is the shuffle: cloud c's segment of the sorted
 * row indices is a permutation of its rows.  Refused: a negative count, NULLs with work to do. */
int regtr_shuffle_keys(const int* seg_off, int n_clouds, int n, unsigned long long seed, unsigned int step, long long* keys,
                       void* stream);

/* The one pass over the points.  Output row j of output cloud slot c' (out_off [n_clouds + 1], out_off[n_clouds] = n_out) reads input
 * row perm[in_off[c] + j] of the input cloud slot c = in_slot[c'] (perm [n_in] int64: global input rows, a permutation within every
 * cloud; NULL: the identity, i.e. the cloud's leading rows), applies xform[c] (3x4, rounded per operation as regtr_se3_transform;
 * xform NULL: no transform, the point is copied) and adds noise z with z three normals of counter (j, c', 2, step) (float32 Box-Muller
 * with the accurate logf / log1pf / sincosf; noise == 0 adds nothing, so -0 stays -0).  out_xyz [n_out, 3]; out_mask [n_out] (optional)
 * = mask[input row].  Rows and slots are clamped to their cloud, so no table can make a read leave the arrays; the caller keeps
 * out_off[c' + 1] - out_off[c'] <= the length of input cloud in_slot[c'].  Refused: a negative count, n_out > n_in, a NaN noise, NULLs
 * with work to do, out_mask without mask. */
int regtr_augment_gather(const float* xyz, const unsigned char* mask, const int* in_off, int n_in, const long long* perm,
                         const int* out_off, const int* in_slot, int n_clouds, int n_out, const float* xform, float noise,
                         unsigned long long seed, unsigned int step, float* out_xyz, unsigned char* out_mask, void* stream);

/* ---- ModelNet training augmentation (regtr_amd/augment.py: modelnet_train_batch; csrc/augment_modelnet.hip) ------------------------- */

/* The chain SplitSourceRef -> RandomCrop -> RandomTransformSE3_euler -> Resampler -> RandomJitter -> ShufflePoints of
 * data_loaders/modelnet.py:102-109 on n_clouds packed raw clouds (xyz [n_raw, 3], raw_off [n_clouds + 1]).  2 n_clouds SLOTS: slot b is
 * the source copy of raw cloud b, slot n_clouds + b its reference copy; slot_off [2 n_clouds + 1] are the exclusive offsets of the slots'
 * raw rows (slot s has the rows of cloud s mod n_clouds; slot_off[2 n_clouds] = n_slot_rows = 2 n_raw).  Random numbers: the Philox
 * convention above with purposes 3-7; csrc/augment_modelnet.hip states which word feeds which decision. */

/* One thread per raw cloud b.  dirs [2 n_clouds, 3]: the crop direction of every slot, uniform on the sphere (float64 trigonometry, rounded
 * to float32).  xform [n_clouds, 3, 4]: R = Rx Ry Rz of three angles u pi rot_mag / 180, t uniform in +-trans_mag, formed in float64 and
 * rounded once to float32; pose [n_clouds, 3, 4] = its inverse [R^T | -R^T t] in float32 rounded per operation.  Refused: a negative
 * count, a NaN magnitude, NULLs with work to do. */
int regtr_modelnet_draws(int n_clouds, unsigned long long seed, unsigned int step, double rot_mag, double trans_mag, float* dirs,
                         float* xform, float* pose, void* stream);

/* The largest cloud whose distance keys regtr_crop_select keeps resident in LDS (host only). */
int regtr_crop_select_lds_points(void);

/* RandomCrop.crop of every slot, one workgroup per slot: centroid [2 n_clouds, 3] (float64 sums in a fixed order, rounded once to
 * float32), distance of a row = float64 dot product of its float32 centred point with the float32 direction dirs[slot] (sums left to
 * right, no contraction; -0 counts as +0), thr [2 n_clouds] (float64) = numpy's linear-interpolation percentile of the distances:
 * with a <= b the order statistics of 0-based ranks sel_lo[slot] and sel_lo[slot] + 1 and t = sel_t[slot], a + (b - a) t for t < 0.5
 * and b - (b - a)(1 - t) otherwise (sel_lo, sel_t: functions of n and p_keep alone, from the host).  keep [n_slot_rows] = distance > thr,
 * strictly; count [2 n_clouds] the rows kept.  A slot that would keep nothing keeps every row instead and gets flag [2 n_clouds] = 1.
 * The order statistics come from an 8-bit radix select on the order-preserving 64-bit keys of the distances, resident in LDS for a cloud
 * of at most min(max_len, regtr_crop_select_lds_points()) rows and recomputed from xyz in every digit pass for a larger one (max_len: the
 * caller's bound on the clouds' lengths; it sizes the LDS and may be wrong without harm).  Bit-reproducible.  A slot whose offsets are
 * not this layout gets count 0 and no other write.  Refused: a negative count, NULLs with work to do. */
int regtr_crop_select(const float* xyz, const int* raw_off, int n_raw, int n_clouds, int max_len, const float* dirs, const int* sel_lo,
                      const double* sel_t, const int* slot_off, int n_slot_rows, float* centroid, double* thr, int* count, int* flag,
                      unsigned char* keep, void* stream);

/* keys [n_slot_rows + n_slots k_out] int64, two families in one array for ONE stable ascending sort:
 *   raw row r of slot s (index slot_off[s] + r):        (s << 32) | (!keep << 31) | (x0 of counter (r, s, 4, step) >> 1)
 *   pre-shuffle output row i of slot s (index n_slot_rows + s k_out + i):   ((n_slots + s) << 32) | x0 of counter (i, s, 6, step)
 * Sorted, slot s's first segment lists its kept rows first, in uniform random order (Resampler); its second segment is ShufflePoints'
 * permutation of its k_out output rows.  Refused: a negative count, 2^31 keys or more, NULLs with work to do. */
int regtr_modelnet_keys(const int* slot_off, int n_slots, int n_slot_rows, int k_out, const unsigned char* keep, unsigned long long seed,
                        unsigned int step, long long* keys, void* stream);

/* The one pass over the 2 n_clouds k_out output rows.  Final row j of slot s reads pre-shuffle row i = perm[n_slot_rows + s k_out + j]
 * (perm: the sorted keys' indices, int64); pre-shuffle row i reads sorted kept row q = i for i < m = count[s], else x0 of counter
 * (i, s, 5, step) mod m (a pick with replacement); that is raw row r = perm[slot_off[s] + q] - slot_off[s] of the slot's cloud.  Source
 * slots go through xform[s] (3x4, rounded per operation as regtr_se3_transform), then every row gains
 * clip(scale z, -clip, clip) with z three normals of counter (j, s, 7, step) (scale == 0 adds nothing).  out_xyz [2 n_clouds k_out, 3];
 * out_mask = keep[raw row r of the OTHER slot of the same cloud] (the ground-truth overlap); out_row = r.  Rows and slots are clamped to
 * their cloud, so no table can make a read leave the arrays.  A slot whose offsets are not this layout (the condition under which
 * regtr_crop_select writes count 0) gets zero points, a zero mask and out_row = -1 in all its rows.  Refused: a negative count, a NaN
 * scale, a negative or NaN clip, 2^31 rows or more, NULLs with work to do. */
int regtr_modelnet_gather(const float* xyz, const int* raw_off, int n_raw, int n_clouds, const int* slot_off, int n_slot_rows, int k_out,
                          const long long* perm, const int* count, const unsigned char* keep, const float* xform, float scale, float clip,
                          unsigned long long seed, unsigned int step, float* out_xyz, unsigned char* out_mask, int* out_row, void* stream);

/* ---- validation / test metrics (regtr_amd/metrics.py; csrc/metrics.hip) --------------------------------------------------------------
 * New entry points only: no existing signature changes, REGTR_ABI_VERSION stays as it is. */

/* Supports per LDS tile of regtr_nearest (host only): a longer support cloud is scanned in several tiles. */
int regtr_nearest_lds_points(void);

/* For every query point the nearest point of the support cloud of the same index, over n_clouds packed ragged clouds: q_xyz [n_q, 3]
 * with q_off [n_clouds + 1], s_xyz [n_s, 3] with s_off [n_clouds + 1]; q_pose / s_pose [n_clouds, 12] (row-major 3x4, optional): the
 * transform applied to cloud c's queries / supports first, ((r0 x + r1 y) + r2 z) + t per row.  d2 [n_q] = (dx dx + dy dy) + dz dz with
 * d = q - s, float32 rounded per operation, no contraction; idx [n_q] (optional) the support's index within its cloud.  The minimum is
 * taken by a strict < over the supports in ascending index: the lowest index wins a tie and a NaN distance never wins; a query with no
 * candidate below +inf (an empty support cloud, every distance NaN or +inf) gets d2 = +inf and idx = -1.  max_q_len: the longest query
 * cloud (it sizes the grid; queries beyond it are not written).  Bit-reproducible.  Offsets are clamped to the arrays.  Refused: a
 * negative count, more than 65535 clouds, NULLs with work to do. */
int regtr_nearest(const float* q_xyz, const int* q_off, int n_q, const float* s_xyz, const int* s_off, int n_s, int n_clouds,
                  int max_q_len, const float* q_pose, const float* s_pose, float* d2, int* idx, void* stream);

/* out [n_clouds] (float64) = the mean of every packed segment of v [n] (off [n_clouds + 1]): float64 sums in a fixed order (one
 * workgroup per cloud, a strided partial per lane, a fixed tree), as regtr_cloud_centroids; bit-reproducible.  An empty segment gives
 * 0.  Refused: a negative count, NULLs with work to do. */
int regtr_segment_mean(const float* v, const int* off, int n_clouds, int n, double* out, void* stream);

/* Registration errors of n_layers x n_pairs predicted poses pred [n_layers n_pairs, 12] against gt [n_pairs, gt_stride] (gt_stride 12
 * or 16 floats per pair, rows 0-2 read), one thread per (layer, pair), in float64 with sums left to right.  out [n_layers n_pairs, 8]:
 *   0 rot_err_deg, 1 trans_err of pred o gt^-1 (the reference's se3_compare: || t_p - R_p R_g^T t_g ||)
 *   2 err_r_deg,   3 err_t     of gt^-1 o pred (ModelNet: || R_g^T (t_p - t_g) ||)
 *   4 t_mse, 5 t_mae over the translation's components;  6 r_mse, 7 r_mae over the extrinsic-xyz Euler angles in degrees,
 *     a = atan2(R21, R22), b = -asin(clamp(R20)), c = atan2(R10, R00) (at gimbal lock finite, but not scipy's convention).
 * composed [n_layers n_pairs, 12] = pred o gt^-1 rounded to float32.  Refused: a negative count, another gt_stride, NULLs with work to
 * do. */
int regtr_pose_metrics(const float* pred, const float* gt, int gt_stride, int n_layers, int n_pairs, double* out, float* composed,
                       void* stream);

/* ---- the optimiser step (regtr_amd/optim.py; csrc/optim.hip) --------------------------------------------------------------------------
 * clip_grad_norm_ + torch.optim.AdamW / Adam (the reference's trainer.py:104-121) over many tensors per launch.  New entry points only:
 * no existing signature changes, REGTR_ABI_VERSION stays as it is. */

/* One tensor of a multi-tensor call, filled on the HOST and read there by the entry points (they pack chunks of
 * regtr_optim_chunk_tensors() tensors into a by-value kernel argument: no device-side table, no copy, nothing kept between calls).
 * p, g, m, v: device pointers to n float32 elements (parameter, gradient, exp_avg, exp_avg_sq), 4-byte aligned; 16-byte alignment of
 * all of them selects the 16-byte loads and stores.  The scalars are the tensor's own (torch keeps a step count per parameter):
 * bias_correction1 = 1 - beta1^t, sqrt_bias_correction2 = sqrt(1 - beta2^t), computed in float64; each is rounded to float32 once. */
typedef struct {
    float* p;
    const float* g;
    float* m;
    float* v;
    long long n;
    double lr, weight_decay, beta1, beta2, eps, bias_correction1, sqrt_bias_correction2;
} regtr_optim_tensor_t;

/* Host only: elements per workgroup (= per float64 partial) of regtr_grad_sumsq; elements per workgroup of regtr_adam_step; tensors
 * per launch. */
int regtr_optim_norm_slice(void);
int regtr_optim_step_slice(void);
int regtr_optim_chunk_tensors(void);

/* First half of the global gradient norm.  Tensor t's gradient g (n elements; p, m, v and the scalars are not read) is cut into
 * ceil(n / regtr_optim_norm_slice()) slices; partials [n_partials] (float64) receives the sum of squares of every slice, tensor after
 * tensor, slice after slice, each summed in float64 in a fixed order that depends on neither the grid nor the pointer's alignment.
 * n_partials must equal the number of slices.  Bit-reproducible.  Refused: negative counts, a wrong n_partials, NULLs with work to do,
 * a pointer that is not 4-byte aligned. */
int regtr_grad_sumsq(const regtr_optim_tensor_t* tensors, int n_tensors, double* partials, long long n_partials, void* stream);

/* Second half: one workgroup adds the partials in float64 in a fixed order; norm_coef [2] (float32, device) = {total_norm =
 * sqrt(sum), clip_coef = min(1, max_norm / (total_norm + 1e-6))} -- torch.nn.utils.clip_grad_norm_'s formula in float32.  max_norm
 * <= 0: no clipping, clip_coef = 1 and the norm is still written.  A NaN norm gives a NaN coefficient (no skip logic here: that is
 * regtr_grad_norm_finish_guarded below).  n_partials == 0 gives a norm of 0.  Refused: a negative count, a NaN max_norm, NULLs. */
int regtr_grad_norm_finish(const double* partials, long long n_partials, float max_norm, float* norm_coef, void* stream);

/* torch's single-tensor AdamW (decoupled != 0) or Adam (decoupled == 0, weight decay added to the gradient) on every tensor, per
 * element in float32 rounded per operation:
 *   g' = g coef;  AdamW: p = p (1 - lr wd);  Adam: g' = g' + wd p
 *   m = beta1 m + (1 - beta1) g';  v = beta2 v + ((1 - beta2) g') g';  p = p - (lr / bc1) (m / (sqrt(v) / sqrt(bc2) + eps))
 * clip_coef: device float32 read by the kernel (regtr_grad_norm_finish's norm_coef + 1), NULL = 1.  g is NOT modified (unlike
 * clip_grad_norm_, which scales .grad in place).  Elements outside [0, n) of every tensor are never touched.  Bit-reproducible.
 * Refused: negative counts, NULLs with work to do, misaligned pointers, bias corrections that are not positive, a negative eps, NaN
 * scalars. */
int regtr_adam_step(const regtr_optim_tensor_t* tensors, int n_tensors, const float* clip_coef, int decoupled, void* stream);

/* ---- the guarded optimiser step (FusedAdamW(skip_nonfinite=True); csrc/optim.hip) -----------------------------------------------------
 * torch's GradScaler / fused-optimiser found_inf behaviour: a step whose gradient is not finite is left out ON THE DEVICE -- no host
 * read, no host decision.  New entry points beside the ones above: no existing signature changes, REGTR_ABI_VERSION stays as it is.
 *
 * THE GUARD WORD: four int32 on the device, {ok, applied_steps, skipped_steps, reserved}, zeroed by the caller once.  It is written by
 * ONE lane of ONE workgroup (regtr_grad_norm_finish_guarded) with ordinary stores -- no atomics -- and read, guard[0] only and once per
 * workgroup, by regtr_adam_step_guarded (and, as a per-micro-batch flag, by regtr_grad_pack_guarded). */

/* One tensor of regtr_adam_step_guarded, filled on the HOST.  p, g, m, v, n as in regtr_optim_tensor_t.  The hyper-parameters stay
 * float64 all the way into the kernel, which forms every float32 scalar itself, each rounded once and in regtr_adam_step's order:
 * (float)(1 - lr wd), (float)wd, (float)beta, (float)(1 - beta), (float)eps and, from the tensor's own step count t on the device,
 * (float)(lr / (1 - beta1^t)) and (float)sqrt(1 - beta2^t), with beta^t formed by binary exponentiation over the integer t (r = 1; while
 * t: if t odd r = r b; b = b b; t >>= 1) -- never the math library's pow -- every product a double-double one (Dekker's, from float64
 * multiplies, adds and subtracts in a fixed order, no fma): within 1 ulp of the correctly rounded power, and a numpy restatement
 * reproduces it bit for bit (plain float64 squarings were up to 5e4 ulp off at t <= 2^20).  step_index: the tensor's entry in the
 * step-count vector; distinct within a call. */
typedef struct {
    float* p;
    const float* g;
    float* m;
    float* v;
    long long n;
    double lr, weight_decay, beta1, beta2, eps;
    int step_index;
} regtr_optim_guarded_tensor_t;

/* Host only: tensors per launch of regtr_adam_step_guarded (fewer than regtr_optim_chunk_tensors(): the entries are larger and the
 * descriptor still travels by value inside the 4 KiB kernel-argument segment). */
int regtr_optim_guarded_chunk_tensors(void);

/* regtr_grad_norm_finish with three changes.  grad_scale: an optional device float32 (NULL = 1) that multiplies the norm BEFORE the
 * clip coefficient is formed: norm_coef = {total_norm = (float)sqrt(sum) grad_scale, clip_coef = min(1, max_norm / (total_norm + 1e-6))}.
 * guard[0] = ok = 1 exactly when (float)sqrt(sum) * grad_scale is finite and grad_scale is finite, else 0; guard[1] += ok; guard[2] +=
 * 1 - ok.  With grad_scale NULL or exactly 1.0, norm_coef has regtr_grad_norm_finish's bits.  A gradient whose elements are all finite
 * but whose float32 norm overflows (3e38 in every element) counts as NON-FINITE: the coefficient could not be formed from it.  Refused:
 * a negative count, a NaN max_norm, NULL partials with n_partials > 0, a NULL norm_coef or guard, pointers that are not 4-byte aligned. */
int regtr_grad_norm_finish_guarded(const double* partials, long long n_partials, float max_norm, const float* grad_scale, float* norm_coef,
                                   int* guard, void* stream);

/* regtr_adam_step under the guard.  guard[0] == 0: returns without writing a single byte of p, m, v, steps or step_scalars.  guard[0]
 * != 0: first steps[step_index] += 1 for every tensor of the call (float32 counts, torch's layout; an empty tensor's too) and the
 * tensor's two per-step scalars from the advanced count (see regtr_optim_guarded_tensor_t) into step_scalars[2 step_index ..], once per
 * tensor; then regtr_adam_step's update with g' = (g grad_scale) clip_coef (grad_scale: device float32, NULL = 1; exactly 1.0 leaves
 * g's bits) and those scalars.  steps [n_steps], step_scalars [2 n_steps]: device float32, the second a workspace the call owns while
 * it runs (nothing is read from it that the call did not write).  g is not modified.  The launches per
 * regtr_optim_guarded_chunk_tensors() tensors: one tiny one for the counts and scalars, one for the update.  Bit-reproducible.  Refused:
 * negative counts, NULLs with work to do (tensors, steps, step_scalars, guard; p, g, m, v of a non-empty tensor), misaligned pointers,
 * a step_index outside [0, n_steps), a negative or NaN eps, NaN lr or weight_decay, a beta outside [0, 1). */
int regtr_adam_step_guarded(const regtr_optim_guarded_tensor_t* tensors, int n_tensors, float* steps, float* step_scalars, long long n_steps,
                            const float* clip_coef, const float* grad_scale, const int* guard, int decoupled, void* stream);

/* out [2 n] (device float32) = for every step count steps[i] (device float32, integer-valued) the two scalars regtr_adam_step_guarded
 * forms from it: {(float)(lr / (1 - beta1^t)), (float)sqrt(1 - beta2^t)} -- the same device function, for tests and restatements.
 * Refused: a negative count, NULLs with n > 0, misaligned pointers. */
int regtr_adam_bias_scalars(double lr, double beta1, double beta2, const float* steps, int n, float* out, void* stream);

/* ---- the cloud bank (regtr_amd/cloud_bank.py, RegTR.encode_clouds / register; csrc/cloud_bank.hip) ------------------------------------
 * A new entry point only: no existing signature changes, REGTR_ABI_VERSION stays as it is. */

/* Packs whole clouds of a bank into a new order, one launch for up to three row arrays.  The bank holds n_bank_clouds packed ragged
 * clouds (bank_seg [n_bank_clouds + 1], n_bank rows in all); destination cloud d (0 <= d < n_dst) is bank cloud cloud_of[d], and its
 * rows go to rows dst_seg[d] ... of the outputs (n_out rows in all; the caller's dst_seg is the running sum of the selected clouds'
 * lengths).  feats -> out_feats and pe -> out_pe are [*, D] rows (pe / out_pe optional: both or neither), xyz -> out_xyz [*, 3] rows
 * (optional likewise).  max_len: the longest selected cloud (the caller knows the lengths; rows of a cloud beyond max_len are not
 * copied).  A wide row moves as D / 4 aligned 16-byte pieces; the xyz rows as single floats.  Every destination row is written once;
 * no atomics, no workspace; bit-reproducible.  cloud_of entries are clamped to the bank and all rows to n_bank / n_out, so no table
 * can make an access leave the arrays.  No selected row (n_dst == 0, n_out == 0 or max_len == 0): nothing is launched and no pointer
 * is looked at (empty arrays often have NULL bases), REGTR_OK.  Refused
 * (REGTR_ERR_ARG, nothing launched): D < 4 or D % 4 != 0, a negative count, n_dst > 65535, pe without out_pe or xyz without out_xyz
 * (or the reverse), a wide array's base that is not 16-byte aligned, NULL feats / out_feats / tables with work to do. */
int regtr_gather_segments(const float* feats, const float* pe, const float* xyz, int D, const int* bank_seg, int n_bank_clouds, int n_bank,
                          const int* cloud_of, const int* dst_seg, int n_dst, int n_out, int max_len, float* out_feats, float* out_pe,
                          float* out_xyz, void* stream);

/* ---- the gradient bucket (regtr_amd/grad_bucket.py; csrc/grad_bucket.hip) -------------------------------------------------------------
 * Gradient accumulation and the payload of data-parallel training's one all-reduce.  New entry points only: no existing signature
 * changes, REGTR_ABI_VERSION stays as it is. */

/* One tensor of regtr_grad_pack, filled on the HOST and read there (chunks of regtr_optim_chunk_tensors() tensors travel to the kernel
 * by value: no device-side table, no copy, nothing kept between calls).  g: device pointer to n float32 elements, 4-byte aligned (16-byte
 * alignment selects the 16-byte loads), or NULL; offset: the tensor's first element in the bucket, a multiple of 4. */
typedef struct {
    const float* g;
    long long n;
    long long offset;
} regtr_bucket_tensor_t;

/* Host only: elements per workgroup of regtr_grad_pack. */
int regtr_grad_pack_slice(void);

/* For every tensor t and element i < n_t of a float32 bucket of n_bucket elements:
 *   accumulate == 0:  bucket[offset_t + i] = scale g_t[i]                                 (g_t NULL: 0)
 *   accumulate != 0:  bucket[offset_t + i] = fmaf(scale, g_t[i], bucket[offset_t + i])    (g_t NULL: nothing is written)
 * Elements of the bucket outside every segment are never written.  One owner per element, no atomics, no workspace, no host wait; the
 * result depends on neither the grid nor a pointer's alignment (bit-reproducible).  Refused (REGTR_ERR_ARG, nothing launched): a
 * negative count, NULL tensors with n_tensors > 0, a NULL bucket with an element to write to, an offset that is not a multiple of 4, a
 * segment outside [0, n_bucket), segments that are not in ascending order or overlap, a bucket that is not 16-byte aligned, a g that is
 * not 4-byte aligned, a NaN scale. */
int regtr_grad_pack(const regtr_bucket_tensor_t* tensors, int n_tensors, float* bucket, long long n_bucket, float scale, int accumulate,
                    void* stream);

/* regtr_grad_pack under a device flag (GradBucket(skip_nonfinite=True)): flag[0] != 0 -- regtr_grad_pack's arithmetic exactly; flag[0]
 * == 0 -- zeros in every segment under assign (accumulate == 0), nothing written under accumulate.  Elements outside every segment are
 * never written, as above.  flag: device int32 (a guard word's ok, from regtr_grad_sumsq + regtr_grad_norm_finish_guarded over the
 * micro-batch's gradients), read once per workgroup.  n_good: an optional device float32 outside every segment (NULL: none); one lane
 * of one workgroup writes n_good = (accumulate ? n_good : 0) + (flag != 0) with ordinary stores -- the count of micro-batches the bucket
 * holds, never scaled; it is written even when no tensor has an element.  Refused: what regtr_grad_pack refuses, a NULL flag, a flag or
 * n_good that is not 4-byte aligned. */
int regtr_grad_pack_guarded(const regtr_bucket_tensor_t* tensors, int n_tensors, float* bucket, long long n_bucket, float scale,
                            int accumulate, const int* flag, float* n_good, void* stream);

/* ---- ICP pose refinement and registration fitness (regtr_amd/refine.py; csrc/icp.hip) -------------------------------------------------
 * Point-to-point ICP on the full-resolution clouds and Open3D-style fitness / inlier_rmse of a pose.  New entry points only: no
 * existing signature changes, REGTR_ABI_VERSION stays as it is. */

/* Host only: source rows per workgroup of regtr_icp_step's accumulate pass (a cloud of n rows has ceil(n / chunk) chunks). */
int regtr_icp_chunk(void);

/* Bytes of regtr_icp_step's workspace: 17 doubles per chunk slot, ceil(max_src_len / chunk) slots per pair.  0 for a negative count. */
size_t regtr_icp_ws_bytes(int n_pairs, int max_src_len);

/* ONE iteration of point-to-point ICP over packed pairs: an accumulate launch and a solve launch, nothing waits for the host.
 *   src_xyz [n_src, 3] with src_off [n_pairs + 1], tgt_off [n_pairs + 1] over n_tgt target rows: source cloud b searches target cloud b.
 *   grid_ws: a cell grid built ONCE by regtr_cellgrid_build over the targets (n_clouds = n_pairs, ns_cap = n_tgt) with
 *   grid_radius * (1 + 1e-6) >= max_dist, and serving every iteration.  max_src_len >= every source cloud's length (rows of a cloud
 *   beyond it are not visited).  pose [n_pairs, 12] float32 (3x4 row-major) is read and written in place.
 * Accumulate: every source row p of a pair that is not done is transformed, y = ((r0 x + r1 y) + r2 z) + t in float32 rounded per
 * operation (regtr_se3_transform's bits), and matched to the nearest target row q of its pair with d2 < max_dist^2 -- d2 in float64 on
 * the widened coordinates, ties to the lower index: regtr_nearest_in_radius's rule, and its index bit for bit.  Matched rows add to the
 * float64 moments n, sum d2, sum p, sum q, sum p q^T with p the ORIGINAL source point; the sums run in a fixed order without atomics
 * (bit-reproducible).  idx [n_src] (optional): the match, -1 when the ball is empty; d2 [n_src] (optional): its float64 d2, +inf when
 * empty.
 * Solve, per pair: fitness = n / n_src_b (0 for an empty source cloud), inlier_rmse = sqrt(sum d2 / n) (0 when n == 0), written with n
 * to stats [n_pairs, 3] (float64).  The pair is DONE -- done[b] = 1, its pose, stats, iters_run and idx / d2 rows never written again by
 * later calls with iter > 0 -- when iter > 0 and |fitness - previous| < rel_fitness and |inlier_rmse - previous| < rel_rmse (the
 * previous call's stats), when n < 3, when the covariance fixes no rotation (min (lam_i + lam_j) <= 2^-23 lam_0, the test of
 * regtr_weighted_procrustes_bwd), or when its pose holds a non-finite entry.  Otherwise pose = the fit of the matches (cov = sum p q^T /
 * n - pbar qbar^T, R with the reflection rule of regtr_weighted_procrustes, t = qbar - R pbar, float64 rounded to float32) -- the
 * absolute pose, nothing is composed -- and iters_run[b] = iter + 1.
 *   iter: the iteration's number.  iter == 0 reads neither done nor the previous stats and writes done, iters_run and every row of idx /
 *   d2; the caller passes 0, 1, 2, ... over the same arrays.  stats_only != 0: the pass writes stats (and idx / d2) of the pairs that
 *   are not done and leaves pose alone -- after the last iteration it gives the stats of the returned pose; with iter == 0 it is
 *   evaluate_registration.
 * n_pairs == 0 or n_src == 0: REGTR_OK, nothing launched or written.  Refused (REGTR_ERR_ARG, nothing launched): a negative count or
 * iter, n_pairs > 65535 (more clouds than a launch over the grid supports), max_src_len < 1 or > n_src, NULL src_xyz / offsets / grid_ws
 * / pose / stats / iters_run / done / ws, max_dist or grid_radius not > 0, a grid built for a smaller radius.  REGTR_ERR_WORKSPACE:
 * grid_ws_bytes below regtr_cellgrid_ws_bytes(n_tgt, n_pairs) or ws_bytes below regtr_icp_ws_bytes(n_pairs, max_src_len). */
int regtr_icp_step(const float* src_xyz, const int* src_off, int n_src, int max_src_len, const int* tgt_off, int n_tgt, int n_pairs,
                   double max_dist, float grid_radius, const void* grid_ws, size_t grid_ws_bytes, float* pose, int iter, int stats_only,
                   double rel_fitness, double rel_rmse, double* stats, int* iters_run, int* done, int* idx, double* d2, void* ws,
                   size_t ws_bytes, void* stream);

/* ---- surface normals and point-to-plane ICP (regtr_amd/refine.py; csrc/icp_plane.hip) -----------------------------------------------
 * New entry points only: no existing signature changes, REGTR_ABI_VERSION stays as it is.  Neither has a workspace or a size query: the
 * arrays below are the caller's, with the stated shapes. */

/* Surface normals of packed clouds: xyz [n, 3] float32 with seg_off [n_clouds + 1]; grid_ws a cell grid built by regtr_cellgrid_build over
 * the SAME rows (ns_cap = n) with grid_radius * (1 + 1e-6) >= radius.  Per point p the points q of its own cloud with float64
 * d2 = (dx dx + dy dy) + dz dz < radius^2 on the widened coordinates (p itself included) add dq = rint((q - p) 2^s), s the largest
 * integer with radius 2^s <= 2^20, to int64 sums: moments [n, 10] (optional) = n | sum dq (3) | sum dq dq^T (xx xy xz yy yz zz).  The
 * sums are exact, so they do not depend on the order in which the grid lists a cell's points: the outputs are bit-reproducible.
 * In float64 then m = S1 / n, C_ab = S2_ab / n - m_a m_b, and the eigen-decomposition of C by the one-sided Jacobi SVD of
 * regtr_weighted_procrustes (l2 >= l1 >= l0).  valid [n] int32 = (n >= 3 and l1 > 2^-40 l2); normals [n, 3] float32 = the unit
 * eigenvector of l0 rounded to float32 (its sign is unspecified), exactly 0 where valid is 0.
 * n == 0: REGTR_OK, nothing launched.  Refused (REGTR_ERR_ARG, nothing launched): n < 0, n_clouds < 1, radius or grid_radius not > 0,
 * a grid built for a smaller radius, NULL seg_off / grid_ws, NULL xyz / normals / valid with n > 0, a pointer that is not aligned to its
 * element (grid_ws: 16 bytes).  REGTR_ERR_WORKSPACE: grid_ws_bytes below regtr_cellgrid_ws_bytes(n, n_clouds). */
int regtr_estimate_normals(const float* xyz, const int* seg_off, int n, int n_clouds, double radius, float grid_radius, const void* grid_ws,
                           size_t grid_ws_bytes, float* normals, int* valid, long long* moments, void* stream);

/* ONE iteration of point-to-plane ICP over packed pairs, two launches as regtr_icp_step and with its arguments where the names agree
 * (the same chunking regtr_icp_chunk(), float32 transform and match rule: idx, n_match, fitness and inlier_rmse are regtr_icp_step's
 * bits for the same pose).  tgt_normals [n_tgt, 3] float32 and tgt_valid [n_tgt] int32: regtr_estimate_normals' outputs for the targets.
 * Accumulate: a match whose target has a valid normal nrm adds, in float64 with y the transformed source point, r = nrm . (y - q) and
 * J = [y x nrm, nrm] to  partial [n_pairs, ceil(max_src_len / chunk), 30] float64 = n_match | sum d2 | n_sys | sum J^T J (the 21 upper
 * entries by rows) | sum J^T r (6), per chunk and in a fixed order; other matches count for n_match and sum d2 only.  Every slot the
 * solve reads was written by this call's accumulate.
 * Solve, per pair: stats [n_pairs, 3] as regtr_icp_step.  The pair is DONE by regtr_icp_step's relative rule and for a non-finite pose,
 * and also when n_sys < 6, or when the LDL^T (float64, no pivoting) of J^T J scaled to unit diagonal meets a pivot <= 2^-23 (one wall
 * fixes no pose).  Otherwise (J^T J) x = -J^T r, dT = (Rz(x2) Ry(x1) Rx(x0), x[3:6]) and pose64 <- dT pose64 on the float64 master pose
 * pose64 [n_pairs, 12]; pose [n_pairs, 12] float32 = its rounding, iters_run = iter + 1.  iter == 0 writes pose64 = pose before
 * anything else, so the caller need not initialise it.  Rows are always transformed with the float32 pose: the stats are those of the
 * returned pose.  A done pair's pose, pose64, stats, iters_run and idx rows are never written again.  stats_only as regtr_icp_step.
 * n_src == 0: REGTR_OK, nothing launched.  Refused (REGTR_ERR_ARG, nothing launched): what regtr_icp_step refuses, n_pairs < 1, NULL
 * pose64 / partial, NULL tgt_normals / tgt_valid with n_tgt > 0, a pointer that is not aligned to its element (grid_ws: 16 bytes).
 * REGTR_ERR_WORKSPACE: grid_ws_bytes below regtr_cellgrid_ws_bytes(n_tgt, n_pairs). */
int regtr_icp_plane_step(const float* src_xyz, const int* src_off, int n_src, int max_src_len, const float* tgt_normals, const int* tgt_valid,
                         const int* tgt_off, int n_tgt, int n_pairs, double max_dist, float grid_radius, const void* grid_ws,
                         size_t grid_ws_bytes, float* pose, double* pose64, int iter, int stats_only, double rel_fitness, double rel_rmse,
                         double* stats, int* iters_run, int* done, int* idx, double* partial, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* REGTR_HIP_H */
