/*
 * hfops.h -- C ABI of libhfops.so: the HeteroFusionRCNN point-cloud hot path as
 * hand-written HIP kernels for MI355X (gfx950 / CDNA4).
 *
 * This is the drop-in boundary.  Each entry point replaces one launcher function that the
 * reference's TF custom-op wrappers declare `extern` in their .cpp and define in their .cu
 * (cited per function).  Argument lists keep the reference's order and meaning; the ABI adds
 *   - a trailing `hf_stream_t stream` (a hipStream_t; NULL = the default stream), and
 *   - an `int` status return (HF_OK / HF_E*), never exit() (the reference exit(-1)s at
 *     interpolate/tf_interpolate_g.cu:82-86 and bev_iou/bev_iou.cpp:14-22).
 *
 * Conventions (same as the reference op boundary):
 *   - every pointer is a DEVICE pointer to a dense row-major buffer owned by the caller;
 *   - nothing here allocates, frees, copies to the host or synchronises; all work is
 *     enqueued on `stream`.  Ops that need scratch take it from the caller
 *     (hf_*_workspace() says how much);
 *   - outputs that the reference zero-/one-fills with cudaMemset inside OpKernel::Compute
 *     (tf_grouping.cpp:204, tf_sampling.cpp:174, tf_interpolate.cpp:91-92,130,178,
 *     bev_iou.cpp:175-176, tf_cropping.cpp:171-176) are initialised INSIDE these functions;
 *   - shape/attribute violations that the reference rejects with OP_REQUIRES return
 *     HF_EINVAL and launch nothing;
 *   - stateless, re-entrant, safe to call from several host threads on different streams.
 *
 * Arithmetic contract: IEEE fp32, no FMA contraction, expressions evaluated in the order the
 * reference writes them; integer outputs are bit-exact with the reference semantics
 * (tie rules documented per function).
 */
#ifndef HFOPS_H
#define HFOPS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HF_OK 0
#define HF_EINVAL (-1)     /* shape / attribute violation (OP_REQUIRES in the reference) */
#define HF_EHIP (-2)       /* a HIP runtime call or launch failed; see hf_last_hip_error() */
#define HF_EWORKSPACE (-3) /* caller-provided workspace missing or too small */

typedef void *hf_stream_t; /* hipStream_t */

/* library / error helpers */
const char *hf_version(void);
const char *hf_strerror(int status);
int hf_last_hip_error(void); /* hipError_t of the last HF_EHIP on this thread */

/* ------------------------------------------------------------------ sampling/ */

/* replaces farthestpointsamplingLauncher(b,n,m,inp,temp,out)  sampling/tf_sampling.cpp:94
 * (kernel sampling/tf_sampling_g.cu:105-170).  inp (b,n,3) -> out (b,m) int32; out[:,0] = 0.
 * Tie rule among equal max-min distances: smallest (k mod 512), then smallest k.
 * `temp` is the reference's (32,n) float scratch; this implementation keeps the running
 * distances on chip when n <= hf_fps_onchip_limit() and then ignores it (may be NULL);
 * above that limit it needs hf_fps_workspace(b,n) bytes there. */
int hf_farthest_point_sample(int b, int n, int m, const float *inp, float *temp, int *out, hf_stream_t stream);
/* The same op with the kernel forced (the tests run every kernel against the oracle): HF_FPS_PLAIN = points and running
 * distances in registers, `threads` = 256 / 512 / 1024 per cloud (0: by size); HF_FPS_BUCKET = the spatially bucketed kernel
 * with exact pruning, `threads` = 1024 (16 waves x 16 buckets) or anything else = 512 (8 waves x 32 buckets, the default);
 * HF_FPS_WAVE = one wave per cloud, no barrier per round (n <= 512: the RoI clouds of the second stage);
 * HF_FPS_AUTO = what hf_farthest_point_sample picks (one wave per cloud up to 512 points, bucketed from 8192).  Identical output
 * whatever the choice. */
#define HF_FPS_AUTO 0
#define HF_FPS_PLAIN 1
#define HF_FPS_BUCKET 2
#define HF_FPS_WAVE 3
int hf_farthest_point_sample_variant(int kernel, int threads, int b, int n, int m, const float *inp, float *temp, int *out,
                                     hf_stream_t stream);
size_t hf_fps_workspace(int b, int n);
int hf_fps_onchip_limit(void);

/* replaces gatherpointLauncher(b,n,m,inp,idx,out)  sampling/tf_sampling.cpp:125 (kernel :172-181) */
int hf_gather_point(int b, int n, int m, const float *inp, const int *idx, float *out, hf_stream_t stream);

/* replaces cudaMemset + scatteraddpointLauncher(b,n,m,out_g,idx,inp_g)  sampling/tf_sampling.cpp:150,174 */
int hf_gather_point_grad(int b, int n, int m, const float *out_g, const int *idx, float *inp_g, hf_stream_t stream);

/* ------------------------------------------------------------------ grouping/ */

/* replaces queryBallPointLauncher(b,n,m,radius,nsample,xyz1,xyz2,idx,pts_cnt)  grouping/tf_grouping.cpp:66
 * (kernel grouping/tf_grouping_g.cu:3-36).  xyz1 (b,n,3) data, xyz2 (b,m,3) queries ->
 * idx (b,m,nsample): the first nsample data indices, ascending, with
 * max(sqrtf(|q-p|^2),1e-20f) < radius; remaining slots repeat the first hit; a query with
 * no hit gets a row of zeros (undefined in the reference).  pts_cnt (b,m) = #hits (<= nsample),
 * may be NULL.  radius > 0 and nsample > 0 required (tf_grouping.cpp:70-74). */
int hf_query_ball_point(int b, int n, int m, float radius, int nsample, const float *xyz1, const float *xyz2,
                        int *idx, int *pts_cnt, hf_stream_t stream);

/* replaces groupPointLauncher(b,n,c,m,nsample,points,idx,out)  grouping/tf_grouping.cpp:142 (kernel :40-57) */
int hf_group_point(int b, int n, int c, int m, int nsample, const float *points, const int *idx, float *out,
                   hf_stream_t stream);

/* replaces cudaMemset + groupPointGradLauncher(...)  grouping/tf_grouping.cpp:173,204 (kernel :61-78) */
int hf_group_point_grad(int b, int n, int c, int m, int nsample, const float *grad_out, const int *idx,
                        float *grad_points, hf_stream_t stream);

/* The CSR inverse of an index tensor, built with the geometry (coordinates only): idx holds `total` values per cloud, each in
 * [0, m) (group_point / kNN tables: total = queries * nsample; three_nn: total = 3 n).  offsets (b, m+1), entries (b, total):
 * for every target the flat positions that name it, ascending.  m <= 19968 (two LDS words per target).
 * hf_group_point_grad_gather: the gradient of hf_group_point / hf_group_point_into over that inverse -- every data point sums
 * the grad_out rows that name it in ascending (query, slot) order (the order of the reference's CPU loop,
 * grouping/test/query_ball_point.cpp:53-66) and its row is written once: no atomics, no zero fill, deterministic.
 * grad_out rows have stride `width`, the gathered columns start at `col` (width = c, col = 0 for plain group_point). */
int hf_index_inverse(int b, long long total, int m, const int *idx, int *offsets, int *entries, hf_stream_t stream);
int hf_group_point_grad_gather(int b, int n, int c, int m, int nsample, int width, int col, const float *grad_out,
                               const int *offsets, const int *entries, float *grad_points, hf_stream_t stream);

/* Fused query_ball_point + group_point(xyz) in ONE launch: the pair of calls at
 * hf/core/feature_extractors/pointnet_util.py:48-49,258-259.  Outputs are exactly those of the
 * two separate ops; grouped_xyz (b,m,nsample,3) optionally has the query subtracted
 * (`center` != 0: pointnet_util.py:50-52, same fp32 subtraction).  idx / pts_cnt may be NULL. */
int hf_query_ball_group_xyz(int b, int n, int m, float radius, int nsample, const float *xyz1, const float *xyz2,
                            int center, int *idx, int *pts_cnt, float *grouped_xyz, hf_stream_t stream);

/* The same op pair with a caller-owned workspace (hf_ball_query_workspace(b, n) bytes, 16-byte aligned) and an explicit
 * kernel choice.  With a workspace the batched shapes of a train step (more workgroups than one round of the single-launch
 * kernel) build the cell structure of every cloud ONCE (counting sort by hashed cell) and answer all query tiles from it.
 * variant: HF_BQ_AUTO by shape, or one kernel forced (HF_BQ_CELL single launch, HF_BQ_BRUTEFORCE, HF_BQ_SORTED) -- the tests
 * run every kernel against the oracle this way.  grouped_xyz may be NULL (query_ball_point alone); outputs identical to
 * hf_query_ball_point / hf_query_ball_group_xyz whatever the variant. */
#define HF_BQ_AUTO 0
#define HF_BQ_CELL 1
#define HF_BQ_BRUTEFORCE 2
#define HF_BQ_SORTED 3
size_t hf_ball_query_workspace(int b, int n);
int hf_query_ball_group_xyz_ws(int variant, int b, int n, int m, float radius, int nsample, const float *xyz1,
                               const float *xyz2, int center, int *idx, int *pts_cnt, float *grouped_xyz, void *workspace,
                               size_t workspace_bytes, hf_stream_t stream);

/* replaces selectionSortLauncher(b,n,m,k,dist,outi,out)  grouping/tf_grouping.cpp:108 (kernel :83-123) */
int hf_select_top_k(int b, int n, int m, int k, const float *dist, int *outi, float *out, hf_stream_t stream);

/* ---------------------------------------------------------------- interpolate/ */

/* replaces three_nn_gpu(b,n,m,unknown,known,dist2,idx)  interpolate/tf_interpolate.cpp:60
 * (kernel interpolate/tf_interpolate_g.cu:22-65).  Three smallest (squared distance, index)
 * pairs per unknown point, earlier index first on ties; unused slots (m<3) = +inf / 0. */
int hf_three_nn(int b, int n, int m, const float *unknown, const float *known, float *dist2, int *idx,
                hf_stream_t stream);

/* replaces three_interpolate_gpu(b,c,m,n,points,idx,weight,out)  tf_interpolate.cpp:99 (kernel :90-110)
 * channel-first: points (b,c,m) -> out (b,c,n) */
int hf_three_interpolate(int b, int c, int m, int n, const float *points, const int *idx, const float *weight,
                         float *out, hf_stream_t stream);

/* replaces cudaMemset + three_interpolate_grad_gpu(b,c,n,m,grad_out,idx,weight,grad_points)
 * tf_interpolate.cpp:141,178 (kernel :133-155); channel-first */
int hf_three_interpolate_grad(int b, int c, int n, int m, const float *grad_out, const int *idx,
                              const float *weight, float *grad_points, hf_stream_t stream);

/* Channel-last forms = what the Python surface interpolate/tf_interpolate.py:26-49 exposes
 * (it transposes (b,m,c)->(b,c,m), calls the op, transposes back).  Same values, no transposes:
 * points (b,m,c) -> out (b,n,c);  grad_out (b,n,c) -> grad_points (b,m,c). */
int hf_three_interpolate_cl(int b, int m, int c, int n, const float *points, const int *idx, const float *weight,
                            float *out, hf_stream_t stream);
int hf_three_interpolate_cl_grad(int b, int n, int c, int m, const float *grad_out, const int *idx,
                                 const float *weight, float *grad_points, hf_stream_t stream);

/* -------------------------------------------------------------------- bev_iou/ */

/* replaces cudaMemset x2 + compute_bev_iou_gpu(num_a,boxes_a,num_b,boxes_b,ans_overlap,ans_iou)
 * bev_iou/bev_iou.cpp:144,175-177 (kernel bev_iou_g.cu:240-254).  boxes (N,5) [x1,y1,x2,y2,ry].
 * ans_overlap / ans_iou (num_a,num_b); either may be NULL.  num_a > 0, num_b > 0 required. */
int hf_compute_bev_iou(int num_a, const float *boxes_a, int num_b, const float *boxes_b, float *ans_overlap,
                       float *ans_iou, hf_stream_t stream);

/* replaces oriented_nms_gpu(boxes,mask,boxes_num,thresh)  bev_iou/bev_iou.cpp:40 (kernel bev_iou_g.cu:256-298)
 * mask (n, ceil(n/64)) uint64, every tile written as in the reference. */
int hf_nms_mask(const float *boxes, unsigned long long *mask, int boxes_num, float nms_overlap_thresh,
                hf_stream_t stream);

/* The whole OrientedNMSOp::Compute (bev_iou.cpp:60-116) without its cudaMalloc / blocking D2H /
 * host sweep / H2D: mask kernel + device-resident greedy sweep.  boxes are score-sorted (N,5);
 * keep (N) int32 = kept indices ascending, tail padded with keep[0]; *num_kept (device int,
 * may be NULL) = count before padding.  thresh >= 0, n > 0 required.
 * Workspace per frame (hf_oriented_nms_workspace(n) bytes, a multiple of 256; the base 16-byte aligned): the dense
 * mask (n * ceil(n/64) words), then -- each part padded to 256 bytes -- one counter per column block, one list of
 * 2048 (word, row) entries per column block (the nonzero words right of the diagonal, what the sweep reads), the
 * n transposed diagonal words, an 80-byte table entry per box (cos / sin / corners, computed once per call) and the n
 * mask words next to the diagonal.  About 1.5x the dense mask at n = 9000 (15.6 MB). */
size_t hf_oriented_nms_workspace(int n);
int hf_oriented_nms(const float *boxes, int n, float thresh, int *keep, int *num_kept, void *workspace,
                    size_t workspace_bytes, hf_stream_t stream);
/* The reference maps OrientedNMS over the frames of a batch with tf.map_fn (rpn_model.py:683-687), i.e. one
 * op call (and one host round trip) per frame.  Batched form: boxes (frames, n, 5), keep (frames, n),
 * num_kept (frames) or NULL, workspace = frames * hf_oriented_nms_workspace(n) bytes; one launch pair. */
int hf_oriented_nms_batched(int frames, const float *boxes, int n, float thresh, int *keep, int *num_kept,
                            void *workspace, size_t workspace_bytes, hf_stream_t stream);

/* ------------------------------------------------------------------- cropping/ */

/* replaces cudaMemset x6 + pccropandsample_gpu(...)  cropping/tf_cropping.cpp:100,171-180
 * (kernel cropping/tf_cropping_g.cu:43-132).  `mask`/`crop_mask`/`non_empty_box` are 1-byte bools.
 * Deterministic: the points of each box are taken in ascending point index (the reference's
 * order is atomic-arrival order; ascending is the member of its output set that a
 * single-thread launch produces).  resize > 0 required; box_ind values must lie in [0,batch). */
int hf_pc_crop_and_sample(const float *pts, const float *fts, const float *intensities, const unsigned char *mask,
                          const float *boxes, const int *box_ind, int num_boxes, int batch, int npts, int resize,
                          int channel, int intensity_channel, float *crop_pts, float *crop_fts,
                          float *crop_intensities, unsigned char *crop_mask, int *crop_ind,
                          unsigned char *non_empty_box, hf_stream_t stream);

/* replaces cudaMemset + pccropandsamplegradfts_gpu(box_ind,crop_ind,grad_crop_fts,num_boxes,npts,resize,channel,grad_fts)
 * cropping/tf_cropping.cpp:192,225.  `batch` added so the zero fill can happen here. */
int hf_pc_crop_and_sample_grad_fts(const int *box_ind, const int *crop_ind, const float *grad_crop_fts,
                                   int num_boxes, int batch, int npts, int resize, int channel, float *grad_fts,
                                   hf_stream_t stream);

/* ------------------------------------------------- callers of the path: the grouped-point MLP */

/* k nearest data points of every query: the knn_point of grouping/tf_grouping.py:62-95 (and PointCNN's
 * knn_indices_general, hf/core/pointfly.py:185-212) without the dense (b,m,n) distance matrix.
 * xyz1 (b,n,3) data, xyz2 (b,m,3) queries -> val (b,m,k) squared distances ascending, idx (b,m,k) int32;
 * equal distances: lower index first (tf.nn.top_k's rule).  1 <= k <= min(n, 67). */
int hf_knn_point(int b, int n, int m, int k, const float *xyz1, const float *xyz2, float *val, int *idx,
                 hf_stream_t stream);

/* Training-mode batch norm (+ optional ReLU) over channel-last rows x (rows, c): the
 * tf_util.batch_norm_template + tf.nn.relu pair inside tf_util.conv2d
 * (hf/core/feature_extractors/tf_util.py:190-203,554-581; decay = 1 - momentum, epsilon = eps).
 * Batch statistics are reduced deterministically (per-block fp32 partials, fp64 final reduction).
 * running_mean / running_var (may be NULL) are updated as (1-momentum)*running + momentum*batch
 * (biased variance, as TensorFlow's moments).  save_mean / save_invstd (c floats each) feed the backward pass.
 * `relu` (all BatchNorm entry points that take it): bit 0 = ReLU after the normalisation; bit 1 = ELU applied to x on
 * load, before the statistics and the normalisation (pointfly.dense / conv2d: linear -> ELU -> batch_normalization,
 * hf/core/pointfly.py:371-497): 0 none, 1 BN+ReLU, 2 ELU+BN.
 * workspace: hf_bn_workspace(rows, c) bytes of device scratch.
 * Channel limit of every hf_bn_* entry point and of hf_narrow_linear_dx (its cin): c <= 4096, and c <= 1024 where c % 4 != 0 (such
 * rows are accessed one float at a time, one thread per channel of a row, and a workgroup holds 1024 threads); anything beyond is
 * HF_EINVAL before a launch.  c % 4 == 0 takes 16-byte accesses and needs 16-byte aligned tensors (and row strides).
 * The batch variance is ONE pass, E[x^2] - mean^2, from per-block fp32 partial sums added in fp64: its absolute error is bounded by
 * c u E[x^2] (u = 2^-24, c = 3 (fp32 additions into one partial) + 1, a few hundred at most), so relative to the variance it grows with
 * 1 + (mean / std)^2 -- measured: at most 0.013 of that bound at mean / std = 30, relative variance errors of 1e-6 to 2.9e-4 (profiles/bn_parity.md);
 * tf.nn.moments, two passes, has no such term.  Feed these entry points roughly centred channels. */
size_t hf_bn_workspace(long long rows, int c);
int hf_bn_relu_fwd_train(long long rows, int c, const float *x, const float *gamma, const float *beta, float eps,
                         float momentum, float *running_mean, float *running_var, int relu, float *y,
                         float *save_mean, float *save_invstd, void *workspace, size_t workspace_bytes,
                         hf_stream_t stream);
/* inference: y = relu?(gamma*invstd*(x-mean)+beta) with caller-provided mean / invstd */
int hf_bn_relu_fwd_eval(long long rows, int c, const float *x, const float *gamma, const float *beta,
                        const float *mean, const float *invstd, int relu, float *y, hf_stream_t stream);
/* backward of hf_bn_relu_fwd_train: dx (rows,c), dgamma (c), dbeta (c); the ReLU mask is recomputed from x.
 * dx_colsum (c floats, may be NULL) receives the column sums of dx: the bias gradient of the Linear / 1x1
 * convolution that produced x, for free in the same pass. */
int hf_bn_relu_bwd(long long rows, int c, const float *x, const float *dy, const float *gamma, const float *beta,
                   const float *save_mean, const float *save_invstd, int relu, float *dx, float *dgamma,
                   float *dbeta, float *dx_colsum, void *workspace, size_t workspace_bytes, hf_stream_t stream);
/* The same two passes with ROW STRIDES on the normalised tensor: y (forward) / dy (backward) may be a column slice of a wider
 * buffer (ld floats per row, ld >= c; 16-byte rows when c % 4 == 0).  That is how a BatchNorm output lands directly inside
 * the concat the reference builds next (pointcnn.py:104, :349: [lifted | gathered], [x-conv | skip]) and how its gradient is
 * read out of the concat's gradient in place: no tf.concat copy in either direction. */
int hf_bn_relu_fwd_train_ld(long long rows, int c, const float *x, const float *gamma, const float *beta, float eps,
                            float momentum, float *running_mean, float *running_var, int relu, float *y, long long ldy,
                            float *save_mean, float *save_invstd, void *workspace, size_t workspace_bytes, hf_stream_t stream);
int hf_bn_relu_bwd_ld(long long rows, int c, const float *x, const float *dy, long long lddy, const float *gamma,
                      const float *beta, const float *save_mean, const float *save_invstd, int relu, float *dx, float *dgamma,
                      float *dbeta, float *dx_colsum, void *workspace, size_t workspace_bytes, hf_stream_t stream);

/* knn_point (see hf_knn_point) with a scratch buffer: the data points of every cloud are binned into a 2-D grid over
 * its two widest axes first; each query then searches rings of cells around its own and stops once everything outside
 * the visited block is provably farther than its k-th best distance.  Same outputs as hf_knn_point (ties to the lower
 * index).  hf_knn_workspace returns 0 for n > 65536; hf_knn_point_sorted then runs hf_knn_point. */
size_t hf_knn_workspace(int b, int n);
int hf_knn_point_sorted(int b, int n, int m, int k, const float *xyz1, const float *xyz2, float *val, int *idx,
                        void *workspace, size_t workspace_bytes, hf_stream_t stream);

/* The concat of sample_and_group (pointnet_util.py:58-60) in one pass: out (b, m, nsample, width) rows are
 * [grouped_xyz (3), points[idx] (c), zeros], or with xyz_last != 0 the multi-scale module's order
 * [points[idx] (c), grouped_xyz (3), zeros] (pointnet_util.py:264); width >= 3 + c, width % 4 == 0.  Replaces
 * group_point + concat.  hf_group_concat_grad scatters the feature columns of grad_out back to grad_points (b, n, c). */
/* group_point into / its gradient out of a column slice of wider rows: out (b, m, nsample, width)[..., col : col + c] =
 * points[idx]; the other columns are not touched.  For concatenations whose other part is produced elsewhere (PointCNN's
 * [lifted coordinates | gathered features], pointcnn.py:96-99).  16-byte copies when c, width, col are multiples of 4. */
int hf_group_point_into(int b, int n, int c, int m, int nsample, int width, int col, const float *points, const int *idx,
                        float *out, hf_stream_t stream);
int hf_group_point_grad_from(int b, int n, int c, int m, int nsample, int width, int col, const float *grad_out,
                             const int *idx, float *grad_points, hf_stream_t stream);
int hf_group_concat(int b, int n, int c, int m, int nsample, int width, int xyz_last, const float *grouped_xyz,
                    const float *points, const int *idx, float *out, hf_stream_t stream);
int hf_group_concat_grad(int b, int n, int c, int m, int nsample, int width, int xyz_last, const float *grad_out,
                         const int *idx, float *grad_points, hf_stream_t stream);

/* three_nn (tf_interpolate.cpp:68-75) with a scratch buffer: the known points of every cloud are binned into a 2-D
 * grid first, each unknown point then searches rings of cells around its own (the k = 3 case of hf_knn_point_sorted).
 * Same outputs as hf_three_nn, bit for bit (ties to the lower index, +inf / 0 when fewer than 3 known points).
 * hf_three_nn_workspace returns 0 for m > 65536; hf_three_nn_sorted then runs hf_three_nn. */
size_t hf_three_nn_workspace(int b, int m);
int hf_three_nn_sorted(int b, int n, int m, const float *unknown, const float *known, float *dist2, int *idx,
                       void *workspace, size_t workspace_bytes, hf_stream_t stream);

/* Inverse of a three_nn index (tf_interpolate.cpp:68-75 produces idx): for every known point the (unknown point,
 * slot) pairs that reference it, as CSR.  offsets (b, m+1) int32, entries (b, 3n) int32 holding unknown*3+slot in
 * ascending order inside each bucket; idx values outside [0, m) are dropped.  m <= 8192. */
int hf_three_nn_inverse(int b, int n, int m, const int *idx, int *offsets, int *entries, hf_stream_t stream);
/* ThreeInterpolateGrad (tf_interpolate.cpp:39-48, 150-167) in gather form over that inverse, channel-last:
 * grad_out (b,n,c), weight (b,n,3) -> grad_points (b,m,c).  No atomics; sums in the order of the reference's
 * sequential loop (ascending unknown point, then slot). */
int hf_three_interpolate_cl_grad_gather(int b, int n, int c, int m, const float *grad_out, const float *weight,
                                        const int *offsets, const int *entries, float *grad_points, hf_stream_t stream);

/* batch statistics only (the first half of hf_bn_relu_fwd_train): mean / invstd of x (rows, c) over rows, running
 * estimates updated.  For callers that apply the normalisation elsewhere (fused into a pooling or a GEMM operand load). */
int hf_bn_stats(long long rows, int c, const float *x, float eps, float momentum, float *running_mean, float *running_var,
                float *save_mean, float *save_invstd, void *workspace, size_t workspace_bytes, hf_stream_t stream);

/* three_interpolate written into the concat of pointnet_fp_module (pointnet_util.py:311-313): out (b, n, width) rows are
 * [interpolated (c), skip (c1), zeros]; width >= c + c1, width % 4 == 0; skip (b, n, c1) may be NULL when c1 == 0.
 * hf_three_interpolate_concat_grad: gradient w.r.t. points from the first c columns of grad_out (b, n, width), gather
 * form over the inverse index (see hf_three_nn_inverse). */
int hf_three_interpolate_concat(int b, int m, int c, int n, int c1, int width, const float *points, const int *idx,
                                const float *weight, const float *skip, float *out, hf_stream_t stream);
int hf_three_interpolate_concat_grad(int b, int n, int c, int m, int width, const float *grad_out, const float *weight,
                                     const int *offsets, const int *entries, float *grad_points, hf_stream_t stream);

/* BN + ReLU + max over the k rows of every group, fused: the tail of a set-abstraction MLP
 * (tf_util.conv2d(..., bn=True) then tf.reduce_max(axis=[2]), pointnet_util.py:156-176).  z is (groups*k, c)
 * pre-BN; pooled is (groups, c).  training != 0: batch statistics are computed here (and the running estimates
 * updated) and written to mean / invstd, argmax (groups, c) bytes records the winning row of each maximum
 * (k <= 255); training == 0: mean / invstd are inputs, argmax may be NULL.  The normalised (groups*k, c)
 * activation is never materialised. */
int hf_bn_relu_maxpool_fwd(long long groups, int k, int c, const float *z, const float *gamma, const float *beta,
                           int training, float eps, float momentum, float *running_mean, float *running_var,
                           float *mean, float *invstd, float *pooled, unsigned char *argmax, void *workspace,
                           size_t workspace_bytes, hf_stream_t stream);
/* backward: dpooled (groups, c) -> dz (groups*k, c), dgamma, dbeta, and optionally the column sums of dz */
int hf_bn_relu_maxpool_bwd(long long groups, int k, int c, const float *z, const float *dpooled,
                           const unsigned char *argmax, const float *gamma, const float *beta, const float *save_mean,
                           const float *save_invstd, float *dz, float *dgamma, float *dbeta, float *dz_colsum,
                           void *workspace, size_t workspace_bytes, hf_stream_t stream);

/* Weight gradient of tf_util.conv2d([1,1]) (tf_util.py:180-203) on channel-last rows: grad_weight (cout, cin) =
 * grad_z^T x, fp32 MFMA, reduction over rows split into chunks whose partial tiles are summed in a fixed order.
 * in_gamma != NULL: x is the previous layer's pre-BN output and relu(bn(x)) is applied while it is staged
 * (in_gamma/in_beta/in_mean/in_invstd are that layer's (cin,) parameters and batch statistics). */
size_t hf_linear_wgrad_workspace(long long rows, int cout, int cin);
int hf_linear_wgrad(long long rows, int cout, int cin, const float *grad_z, const float *x, const float *in_gamma,
                    const float *in_beta, const float *in_mean, const float *in_invstd, float *grad_weight,
                    void *workspace, size_t workspace_bytes, hf_stream_t stream);

/* tf_util.conv2d([1,1], bn=True) up to the batch statistics, one pass (tf_util.py:180-203, 554-581):
 * z (rows, cout) = act(x) weight^T + bias on the fp32 MFMA, and the BatchNorm statistics of z (mean, invstd; running
 * estimates updated) from the accumulators.  in_gamma != NULL: x is the PREVIOUS layer's pre-BN output and
 * act = relu(bn(.)) with that layer's (cin,) parameters / statistics is applied while x is staged, so the normalised
 * activation between two layers is not read back; in_gamma == NULL: x is used as is.  x_act (rows, cin), optional
 * with in_gamma: the activated input is also stored (the weight gradient of this layer needs it in training).
 * cout <= 256, cin <= 1024. */
size_t hf_linear_bn_fwd_workspace(int cout);
int hf_linear_bn_fwd(long long rows, int cin, int cout, const float *x, const float *in_gamma, const float *in_beta,
                     const float *in_mean, const float *in_invstd, float *x_act, const float *weight, const float *bias,
                     float *z,
                     float eps, float momentum, float *running_mean, float *running_var, float *mean, float *invstd,
                     void *workspace, size_t workspace_bytes, hf_stream_t stream);

/* The same pass for PointCNN's layer order, pf.dense = linear (no bias) -> ELU -> BatchNorm (pointfly.py:480-497): z is the
 * pre-activation output, the statistics are those of elu(z), and with in_gamma != NULL x is the previous dense layer's
 * pre-activation output with a (elu(x) - mean) + beta applied while it is staged (x_act: stored as well). */
int hf_linear_elu_bn_fwd(long long rows, int cin, int cout, const float *x, const float *in_gamma, const float *in_beta,
                         const float *in_mean, const float *in_invstd, float *x_act, const float *weight, float *z, float eps,
                         float momentum, float *running_mean, float *running_var, float *mean, float *invstd, void *workspace,
                         size_t workspace_bytes, hf_stream_t stream);
/* ... and its input gradient: dx (rows, cin) = dz (rows, cout) W with the BatchNorm-backward sums of the dense layer BELOW
 * (p_dgamma = sum dx * xhat, p_dbeta = sum dx, xhat from elu(z_prev)) taken from the accumulators; workspace as
 * hf_linear_bn_bwd_workspace(cin). */
int hf_linear_elu_bn_bwd(long long rows, int cout, int cin, const float *dz, const float *weight_t, float *dx, const float *z_prev,
                         const float *p_gamma, const float *p_beta, const float *p_mean, const float *p_invstd, float *p_dgamma,
                         float *p_dbeta, void *workspace, size_t workspace_bytes, hf_stream_t stream);

/* The lifting chain of an X-Conv (pointcnn.py:96-99), two pf.dense layers on the local coordinates: x3 (rows, 3) ->
 * y0 = BN0(elu(x3 W0^T)) (c0 channels) -> z1 = y0 W1^T (c1 channels; the caller normalises elu(z1) with mean1 / invstd1).
 * The first layer's output is never stored: its statistics come from one pass over x3, and the second GEMM rebuilds y0 from x3
 * while it stages its operand.  w0 (c0, 3), w1 (c1, c0); batch statistics and running estimates of both layers are produced.
 * hf_lift_elu_bn_bwd: from dz1 (rows, c1) = the gradient w.r.t. z1: grad_w1 (c1, c0), dgamma0 / dbeta0 (c0), and grad_w0_t (3, c0) =
 * the TRANSPOSE of the first layer's weight gradient; dy0 = dz1 W1 (w1_t = W1^T as (c0, c1)) is rebuilt in the accumulators of
 * two passes and never written.  c0 a multiple of 4, c1 <= 256, w1 16-byte aligned (it is read four floats at a time);
 * c0 <= 256 for hf_lift_elu_bn_fwd and the two inference forms below, c0 <= 160 for hf_lift_elu_bn_bwd.  Anything else is HF_EINVAL. */
size_t hf_lift_elu_bn_fwd_workspace(int c0, int c1);
int hf_lift_elu_bn_fwd(long long rows, int c0, int c1, const float *x3, const float *w0, const float *gamma0, const float *beta0,
                       float eps0, float momentum0, float *running_mean0, float *running_var0, float *mean0, float *invstd0,
                       const float *w1, float *z1, float eps1, float momentum1, float *running_mean1, float *running_var1,
                       float *mean1, float *invstd1, void *workspace, size_t workspace_bytes, hf_stream_t stream);
/* inference form: the first layer normalised with the GIVEN mean0 / invstd0 (its running estimates), z1 only; workspace as
 * hf_lift_elu_bn_fwd_workspace */
int hf_lift_elu_fwd_eval(long long rows, int c0, int c1, const float *x3, const float *w0, const float *gamma0, const float *beta0,
                         const float *mean0, const float *invstd0, const float *w1, float *z1, void *workspace, size_t workspace_bytes,
                         hf_stream_t stream);
/* the same with the SECOND layer's inference constants given too: y1 = gamma1 * invstd1 * (elu(z1) - mean1) + beta1 leaves the GEMM's
 * epilogue, the normalisation pass of that layer does not run (two-stage inference: the lifting layers of the RoI clouds) */
int hf_lift_elu_fwd_eval_bn(long long rows, int c0, int c1, const float *x3, const float *w0, const float *gamma0, const float *beta0,
                            const float *mean0, const float *invstd0, const float *w1, const float *gamma1, const float *beta1,
                            const float *mean1, const float *invstd1, float *y1, void *workspace, size_t workspace_bytes,
                            hf_stream_t stream);
size_t hf_lift_elu_bn_bwd_workspace(long long rows, int c0, int c1);
int hf_lift_elu_bn_bwd(long long rows, int c0, int c1, const float *x3, const float *w0, const float *gamma0, const float *beta0,
                       const float *mean0, const float *invstd0, const float *dz1, const float *w1_t, float *grad_w0_t,
                       float *grad_w1, float *dgamma0, float *dbeta0, void *workspace, size_t workspace_bytes, hf_stream_t stream);
/* hf_lift_elu_bn_bwd with dy0 = dz1 W1 formed ONCE (csrc/lift_bwd.hip): the same arguments and outputs.  One sweep over dz1 keeps
 * eleven sums per first-layer channel -- sum dy0, sum dy0 xhat0 and, with s = elu'(z0) and d = 0, 1, 2, A_d = sum dy0 (s x_d),
 * B_d = sum s x_d, C_d = sum xhat0 (s x_d) -- and a finalize kernel adds the workgroups' partials in fp64 and evaluates
 *   grad_w0_t[d][c] = gamma0_c invstd0_c (A_d - (dbeta0_c / rows) B_d - (dgamma0_c / rows) C_d)
 * in fp64, rounded once.  grad_w1, dgamma0 and dbeta0 are bit-identical to hf_lift_elu_bn_bwd's; grad_w0_t agrees with it to fp32
 * rounding of the sums (no atomics: two calls give the same bits).  c0 a multiple of 4 and <= 128 (wider chains: hf_lift_elu_bn_bwd),
 * c1 <= 256; anything else is HF_EINVAL, a missing or short workspace HF_EWORKSPACE, both before any launch. */
size_t hf_onepass_lift_elu_bn_bwd_workspace(long long rows, int c0, int c1);
int hf_onepass_lift_elu_bn_bwd(long long rows, int c0, int c1, const float *x3, const float *w0, const float *gamma0, const float *beta0,
                               const float *mean0, const float *invstd0, const float *dz1, const float *w1_t, float *grad_w0_t,
                               float *grad_w1, float *dgamma0, float *dbeta0, void *workspace, size_t workspace_bytes,
                               hf_stream_t stream);

/* Reduced-precision inference of the wide dense layers (csrc/linear_bf16.hip): the only entry points of the library that do not
 * compute in fp32 end to end.  bf16 values travel as uint16_t (the upper half of the fp32 bit pattern).
 * fp32 -> bf16, round to nearest even; the same device function the GEMM applies to x while staging.  n >= 1.  A value whose
 * magnitude rounds past the largest finite bf16 becomes Inf; NaN stays NaN.  Inputs below the fp32 normal range (subnormals) are
 * outside the contract of both entry points: the hardware conversion may flush them. */
int hf_f32_to_bf16(long long n, const float *src, uint16_t *dst, hf_stream_t stream);

/* inference only: z = bf16(x) (rows, cin) . w_bf16^T (cout, cin), products exact, accumulated in fp32, + bias (may be NULL);
 * with gamma/beta/mean/invstd given (all four or none): y = relu?(gamma * invstd * (elu?(z) - mean) + beta), the convention of
 * hf_bn_relu_fwd_eval / hf_lift_elu_fwd_eval_bn; mode = (1: ReLU) | (2: ELU on z), 0 when the four are NULL.  y is fp32.
 * rows >= 1 (rows / 128 row blocks times the column tiles must fit a 31-bit grid), cin % 4 == 0, cout % 4 == 0, x, w_bf16 and y
 * 16-byte aligned; anything else is HF_EINVAL before a launch.  The ELU is the exp2 form of the streaming BatchNorm passes, the
 * affine is evaluated in their order (difference first), so this call and GEMM + hf_bn_relu_fwd_eval differ only through z. */
int hf_linear_bf16_fwd_eval(long long rows, int cin, int cout, const float *x, const uint16_t *w_bf16, const float *bias,
                            const float *gamma, const float *beta, const float *mean, const float *invstd, int mode,
                            float *y, hf_stream_t stream);

/* Training of the same layers on the bf16 matrix cores (csrc/linear_bf16_train.hip).  The forward z = bf16(x) bf16(W)^T is
 * hf_linear_bf16_fwd_eval with mode 0 and no bias; the two entry points below supply the backward products.  Tensors stay fp32 in
 * memory, accumulation is fp32.
 * dst (cols, rows) = bf16(src (rows, cols))^T, the rounding of hf_f32_to_bf16 (the same device function), through an LDS tile: reads
 * and writes are both coalesced.  With src = W (cout, cin) it yields Wt_bf16 (cin, cout), and the input gradient
 * dx (rows, cin) = bf16(g) (rows, cout) . W is hf_linear_bf16_fwd_eval(rows, cout, cin, g, Wt_bf16, NULL ..., 0, dx): the roles of cin
 * and cout swapped.  rows, cols >= 1 (the 32 x 32 tiles must fit a 31-bit grid), src 4-byte and dst 2-byte aligned; anything else is
 * HF_EINVAL before a launch. */
int hf_f32_to_bf16_transpose(int rows, int cols, const float *src, uint16_t *dst, hf_stream_t stream);

/* grad_weight[o][i] = sum over r of bf16(grad_z[r][o]) * bf16(x[r][i]): both operands are fp32 in memory and rounded (nearest even)
 * while they are staged, as hf_linear_bf16_fwd_eval rounds x; products exact, accumulated in fp32.  The reduction over rows is cut
 * into chunks whose partial tiles go to the workspace and are summed in a fixed order (the convention of hf_linear_wgrad; a single
 * chunk writes grad_weight directly): no floating-point atomics, two calls on the same inputs return the same bits; nothing allocates
 * or synchronises.  rows >= 1, 4 <= cout, cin <= 32768, cout % 4 == 0, cin % 4 == 0, grad_z, x, grad_weight and workspace 16-byte
 * aligned, workspace of at least hf_linear_bf16_wgrad_workspace(rows, cout, cin) bytes (0 for a shape outside the contract);
 * anything else, a missing or short workspace included, is HF_EINVAL before a launch. */
size_t hf_linear_bf16_wgrad_workspace(long long rows, int cout, int cin);
int hf_linear_bf16_wgrad(long long rows, int cout, int cin, const float *grad_z, const float *x, float *grad_weight, void *workspace,
                         size_t workspace_bytes, hf_stream_t stream);

/* BatchNorm (training mode) with the DROPOUT that follows it fused in -- pointfly's dense -> dropout of the PointCNN fc layers and of
 * the RPN box head (hf/core/feature_extractors/pointcnn.py:371-384, hf/core/models/rpn_model.py:556-568: tf.layers.dropout keeps an
 * element with probability 1 - rate and scales it by 1 / (1 - rate)).  y = dropout(bn(act(x))).  The keep decision of an element
 * is a counter hash of (seed of the call, element index), evaluated in the apply pass and again in the two backward passes: no
 * mask tensor, no pass of its own in either direction.  drop_state (device, two 64-bit words: base seed, forward calls so far) belongs
 * to the layer and is advanced on the device (so a captured step draws new masks at every replay); seed_out (device, one word)
 * receives this call's seed and is what hf_bn_dropout_bwd takes.  salt: mixed into the seed (the caller's rank: ranks share the
 * base seed after the parameter broadcast).  0 <= rate < 1, resolved to 1 / 65536.  Other arguments as hf_bn_relu_fwd_train / _bwd. */
int hf_bn_dropout_fwd_train(long long rows, int c, const float *x, const float *gamma, const float *beta, float eps, float momentum,
                            float *running_mean, float *running_var, int relu, float rate, unsigned long long salt,
                            unsigned long long *drop_state, unsigned long long *seed_out, float *y, float *save_mean,
                            float *save_invstd, void *workspace, size_t workspace_bytes, hf_stream_t stream);
int hf_bn_dropout_bwd(long long rows, int c, const float *x, const float *dy, const float *gamma, const float *beta,
                      const float *save_mean, const float *save_invstd, int relu, float rate, const unsigned long long *seed,
                      float *dx, float *dgamma, float *dbeta, void *workspace, size_t workspace_bytes, hf_stream_t stream);

/* Input gradient of a Linear with a handful of outputs (the segmentation head of the RPN, hf/core/models/rpn_model.py: dense to
 * classes + 1 logits): dx (rows, cin) = g (rows, cout) w (cout, cin), 1 <= cout <= 4, cin within the channel limit of the hf_bn_* entry
 * points (above), one streaming pass. */
int hf_narrow_linear_dx(long long rows, int cin, int cout, const float *g, const float *w, float *dx, hf_stream_t stream);

/* The second half of hf_bn_relu_bwd alone: dx from dy, x and ALREADY KNOWN dgamma / dbeta (no reduction pass). */
int hf_bn_relu_bwd_dx(long long rows, int c, const float *x, const float *dy, const float *gamma, const float *beta,
                      const float *save_mean, const float *save_invstd, const float *dgamma, const float *dbeta, int relu,
                      float *dx, hf_stream_t stream);
/* Input gradient of tf_util.conv2d([1,1], bn=True) on the fp32 MFMA: dx (rows, cin) = dz (rows, cout) W, weight_t = W^T
 * as (cin, cout).  z != NULL: the first operand is dy, the gradient w.r.t. this layer's activation, and dz is rebuilt
 * from (dy, z, gamma, beta, mean, invstd, dgamma, dbeta) while it is staged (and stored to dz_out if given); z == NULL:
 * the first operand is dz itself.  z_prev != NULL: dgamma / dbeta of the layer below (p_*: its parameters and
 * statistics, z_prev (rows, cin) its pre-BN output) are reduced from the accumulators into p_dgamma / p_dbeta.
 * dx may be NULL when only dz_out / the sums are wanted.  cin <= 256; cout <= 256 with z, no limit on cout without z
 * (hf_linear_elu_bn_bwd takes no z: cin <= 256 only). */
size_t hf_linear_bn_bwd_workspace(int cin);
int hf_linear_bn_bwd(long long rows, int cout, int cin, const float *dy_or_dz, const float *z, const float *gamma,
                     const float *beta, const float *mean, const float *invstd, const float *dgamma, const float *dbeta,
                     float *dz_out, const float *weight_t, float *dx, const float *z_prev, const float *p_gamma,
                     const float *p_beta, const float *p_mean, const float *p_invstd, float *p_dgamma, float *p_dbeta,
                     void *workspace, size_t workspace_bytes, hf_stream_t stream);

/* ---- glue either side of the ops ---- */

/* The LiDAR -> image fusion step in one pass: hf/core/projection.py:5-32 (tf_rect_to_image: homogeneous point times
 * the 3x4 P2 matrix, divide by depth) + hf/core/models/rpn_model.py:227-235 (tf.cast to int32, tf.gather_nd of the
 * image feature map at [b, v, u]).  pts (b,p,3), calib (b,3,4), img (b,h,w,c) -> out (b,p,c); a pixel outside the
 * image gives zeros (tf.gather_nd on GPU).  pix (b,p,2) [u,v], optional, is what the gradient needs.
 * A quotient outside (-2^31, 2^31) or NaN has no int cast: pix = (-1, -1), a zero row.
 * hf_project_gather_grad: grad_img (b,h,w,c), zero-filled here, += grad_out rows at their pixels; a NULL grad_out or
 * pix with b * p > 0 is HF_EINVAL before grad_img is touched. */
int hf_project_gather(int b, int p, int h, int w, int c, const float *pts, const float *calib, const float *img, float *out,
                      int *pix, hf_stream_t stream);
int hf_project_gather_grad(int b, int p, int h, int w, int c, const float *grad_out, const int *pix, float *grad_img,
                           hf_stream_t stream);
/* The two image-feature gradients in ORDERED form (csrc/ordered_scatter.h): the same sums as hf_project_gather_grad and
 * hf_crop_and_resize_grad, with the order of every sum fixed, so that the result is bit-reproducible.  Both are one operation:
 * E entries in a fixed order, each with a target row key[e] of the (b*h*w, c) map or none and a term of c floats;
 *   grad_img[t] = sum over { e : key[e] == t } of term[e], added in ASCENDING e, in fp32, from +0.0f, one rounding per add:
 * bit for bit what `for e in range(E): if valid[e]: g[key[e]] += term[e]` gives on a zero-filled float32 array.  A target
 * that no entry names becomes +0.0f; every element of grad_img is written by the call (it need not be initialised).
 *   project_gather   entry e = bb*p + point; valid when the saved pix [u,v] lies in [0,w) x [0,h); key = (bb*h + v)*w + u;
 *                    term = grad_out[e, :].
 *   crop_and_resize  entry e = ((r*crop_h + i)*crop_w + j)*4 + tap, taps in the order tl, tr, bl, br; valid exactly where
 *                    hf_crop_and_resize_grad adds (sample inside the image, box finite, box_ind in [0,b); box_ind need not be
 *                    sorted); terms as there, fp32 without contraction: dtop = (1-ly) g, dbot = ly g; tl = (1-lx) dtop,
 *                    tr = lx dtop, bl = (1-lx) dbot, br = lx dbot.  Where floor == ceil two taps of a sample name one pixel:
 *                    both are entries, in tap order.
 * No floating-point atomics; integer atomics only for counts and for slot claims that are sorted afterwards.  No workgroup
 * waits on another.  `workspace`: caller-owned, hf_*_grad_ordered_workspace(shapes) bytes, 16-byte aligned; its counters are
 * zeroed by a kernel on the stream, so the calls can be captured and replayed.  Lists of any length are sorted by a workgroup
 * in O(n log^2 n / 1024): all entries of a frame on one pixel stay in the milliseconds.
 * b == 0 returns HF_OK; p == 0 / n == 0 with a non-empty map writes zeros.  HF_EINVAL: a negative size, h, w, c or crop < 1,
 * b*h*w or E beyond INT_MAX, a NULL required pointer of a non-empty tensor, a workspace that is NULL, misaligned or smaller
 * than asked for.  The workspace functions return 0 for shapes the entries reject and for b == 0. */
size_t hf_project_gather_grad_ordered_workspace(int b, int p, int h, int w, int c);
int hf_project_gather_grad_ordered(int b, int p, int h, int w, int c, const float *grad_out, const int *pix, float *grad_img,
                                   void *workspace, size_t workspace_bytes, hf_stream_t stream);
size_t hf_crop_and_resize_grad_ordered_workspace(int b, int h, int w, int c, long long n, int crop_h, int crop_w);
int hf_crop_and_resize_grad_ordered(int b, int h, int w, int c, long long n, int crop_h, int crop_w, const float *grad_out,
                                    const float *boxes_yxyx, const int *box_ind, float *grad_img, void *workspace,
                                    size_t workspace_bytes, hf_stream_t stream);
/* The image half of the second stage's RoI pooling (hf/core/models/rcnn_model.py:433-454, 494-501), csrc/roi_image.hip.
 * hf_roi_image_boxes: hf/core/projection.py:35-96 (tf_project_to_image_space).  boxes3d (b,n,7) [x,y,z,l,w,h,ry], y at the
 * bottom; calib (b,3,4) P2; h, w the image size the rectangle is normalised by.  The eight corners times P2, divided by depth,
 * min and max over the corners: box_px (b*n,4) [x1,y1,x2,y2] in pixels, box_norm the same divided by [w,h,w,h], box_yxyx
 * box_norm as [y1,x1,y2,x2] (anchor_projector.reorder_projected_boxes); each output may be NULL.  No clipping, no special case
 * for corners behind the camera; a NaN corner gives a NaN rectangle.  b*n <= INT_MAX / 8.
 * hf_crop_and_resize: tf.image.crop_and_resize (bilinear).  img (b,h,w,c), boxes_yxyx (n,4) normalised, box_ind (n) ->
 * out (n,crop_h,crop_w,c).  Sample i sits at in_y = y1 (h-1) + i ((y2-y1) (h-1) / (crop_h-1)), or 0.5 (y1+y2) (h-1) when
 * crop_h == 1 (the same in x), in fp32 in this order.  Inside 0 <= in_y <= h-1 and 0 <= in_x <= w-1: top = tl + (tr-tl) lx,
 * bot = bl + (br-bl) lx, out = top + (bot-top) ly over the floor / ceil neighbours; outside (a NaN is outside), and in every
 * row whose box_ind is not in [0,b): `extrapolation`.
 * hf_crop_and_resize_grad: grad_img (b,h,w,c), zero-filled here (by a kernel on the stream), += the four weighted shares of every in-range sample of
 * grad_out (n,crop_h,crop_w,c), by fp32 atomics (the sum order is not fixed); samples outside and rows with a bad box_ind add
 * nothing.  The coordinates are recomputed as in the forward; there is no gradient w.r.t. the boxes.
 * All three: no workspace, no host round trip, capturable.  n == 0 or b == 0 launch nothing (the gradient still zero-fills a
 * non-empty grad_img).  HF_EINVAL: a negative size, h, w, c or crop < 1, a NULL required pointer of a non-empty tensor, a
 * tensor of more than LLONG_MAX / 4 elements. */
int hf_roi_image_boxes(int b, int n, int h, int w, const float *boxes3d, const float *calib, float *box_px, float *box_norm,
                       float *box_yxyx, hf_stream_t stream);
int hf_crop_and_resize(int b, int h, int w, int c, long long n, int crop_h, int crop_w, const float *img,
                       const float *boxes_yxyx, const int *box_ind, float extrapolation, float *out, hf_stream_t stream);
int hf_crop_and_resize_grad(int b, int h, int w, int c, long long n, int crop_h, int crop_w, const float *grad_out,
                            const float *boxes_yxyx, const int *box_ind, float *grad_img, hf_stream_t stream);
/* The image pyramid's inference kernels (inference.ImgVggPyr in eval mode, image_pyramid.py), csrc/conv_nhwc.hip.  All tensors
 * fp32, dense channel-last, passed as rows of pixels; row and byte offsets are 64-bit, b*h*w <= INT_MAX (INT_MAX / 4 for the
 * up-convolution).
 * hf_conv3x3_nhwc: x (b,h,w,cin); wt (9,cout,cin), tap t = 3 ky + kx, each tap an (N, K) matrix.  z[p,:] = sum over t of
 * x'[src(p,t),:] wt[t]^T with src = (oy + ky - 1, ox + kx - 1) in the same image; a tap outside the image adds zero and is not
 * read.  in_sub: cin floats or NULL; x' = x - in_sub on the elements inside the image only, the padding stays zero.  Epilogue:
 * y = z * scale + shift per output channel (NULL: 1 / 0; multiply and add rounded separately), then max(., 0) if `relu`; y goes to
 * columns [y_col, y_col + cout) of rows y_stride wide, one row per pixel, the other columns are not touched.  The MFMA is
 * v_mfma_f32_32x32x2_f32 over the flattened (tap, channel) axis in a fixed order: two calls give the same bits.
 * hf_upconv3x3s2_nhwc: ConvTranspose2d(3, stride 2, padding 1, output_padding 1): x (b,h,w,cin) -> y (b,2h,2w,cout) with the same
 * epilogue and column slice; wt[3 ky + kx][co][ci] = the module's weight[ci,co,ky,kx].  Input pixel iy feeds output row
 * 2 iy - 1 + ky (the same in x): an even row takes ky = 1, an odd row ky = 0 from iy = (oy+1)/2 if < h and ky = 2 from (oy-1)/2.
 * One launch, one pass per output parity class over its 1, 2, 2 or 4 taps; no MFMA work for a tap that does not exist.
 * hf_maxpool2x2_nhwc: y (b,h/2,w/2,c) dense = the maximum over each 2x2 window (a NaN wins, as torch) of columns
 * [x_col, x_col + c) of x's rows, x_stride wide; a last odd row or column is dropped; h or w == 1 launches nothing.
 * All three: no workspace, no allocation, no host round trip, capturable.  HF_EINVAL before any HIP call: b, h, w, cin (c) < 1,
 * cout outside 1..256, a negative column, a slice that does not fit the stride, b*h*w beyond the limit, a NULL x, wt or y. */
int hf_conv3x3_nhwc(int b, int h, int w, int cin, int cout, const float *x, const float *in_sub, const float *wt,
                    const float *scale, const float *shift, int relu, float *y, int y_stride, int y_col, hf_stream_t stream);
int hf_upconv3x3s2_nhwc(int b, int h, int w, int cin, int cout, const float *x, const float *wt, const float *scale,
                        const float *shift, int relu, float *y, int y_stride, int y_col, hf_stream_t stream);
int hf_maxpool2x2_nhwc(int b, int h, int w, int c, const float *x, int x_stride, int x_col, float *y, hf_stream_t stream);
/* The same two convolutions on the bf16 matrix cores, inference only (image_pyramid.image_precision("bf16")),
 * csrc/conv_nhwc_bf16.hip.  Semantics of hf_conv3x3_nhwc / hf_upconv3x3s2_nhwc: tap numbering, zero padding, in_sub not applied
 * to the padding, the parity classes with their 1, 2, 2 and 4 taps, y = z * scale + shift rounded in two steps, relu, the column
 * slice, the limits and the HF_EINVAL cases (before any HIP call).  Two differences.  Weights: wt_bf16 (9,cout,cin) bf16, the fp32
 * tap matrices passed through hf_f32_to_bf16.  Activation operand: bf16(fl32(x - in_sub)) inside the image and zero outside -- one
 * fp32 subtraction, then the packed hardware conversion (nearest even), between the global load and the LDS store.  x, scale,
 * shift and y stay fp32 in memory; products of two bf16 values are exact in fp32 and accumulate in fp32
 * (v_mfma_f32_16x16x32_bf16) over the flattened (tap, channel) axis in a fixed order: two calls give the same bits.  Any cin, any
 * cout in 1..256, any y_col / y_stride: cin % 4 == 0 with x 16-byte and wt_bf16 8-byte aligned loads quads, anything else takes a
 * scalar staging path; y is stored 16 bytes at a time where cout, y_col, y_stride are multiples of 4 and y is 16-byte aligned.
 * No workspace, no allocation, no host round trip, no environment variable: capturable. */
int hf_conv3x3_nhwc_bf16(int b, int h, int w, int cin, int cout, const float *x, const float *in_sub, const uint16_t *wt_bf16,
                         const float *scale, const float *shift, int relu, float *y, int y_stride, int y_col, hf_stream_t stream);
int hf_upconv3x3s2_nhwc_bf16(int b, int h, int w, int cin, int cout, const float *x, const uint16_t *wt_bf16, const float *scale,
                             const float *shift, int relu, float *y, int y_stride, int y_col, hf_stream_t stream);
/* The image pyramid's training direction (image_pyramid.forward_train), csrc/conv_nhwc.hip.  Same tensors, same limits, same
 * argument checks as the three entry points above (HF_EINVAL before any HIP call); no allocation, no host round trip, no
 * floating-point atomic, capturable; two calls on the same inputs give the same bits.
 * hf_conv3x3s2_nhwc: the adjoint of hf_upconv3x3s2_nhwc and its input gradient.  x (b,2h,2w,cin) -> y (b,h,w,cout): output pixel
 * (oy,ox) sums x[2 oy - 1 + ky, 2 ox - 1 + kx,:] wt[3 ky + kx]^T over the nine taps, zero outside the image; wt (9,cout,cin);
 * epilogue and column slice as hf_conv3x3_nhwc; b*h*w <= INT_MAX / 4.  With wt[t][ci][co] = the up-convolution's wt[t][co][ci] and
 * x = dz it returns that layer's dx.  (The plain convolution's input gradient is hf_conv3x3_nhwc itself on dz with
 * w[t][ci][co] = wt[8 - t][co][ci].)
 * hf_conv3x3_nhwc_wgrad: x (b,h,w,cin), dz (b,h,w,cout) -> dwt (9,cout,cin), dwt[t][co][ci] = sum over pixels p of
 * dz[p][co] x'[p + tap_t][ci], t = 3 ky + kx, tap_t = (ky - 1, kx - 1); x' = x - in_sub (cin floats or NULL) inside the image and zero
 * in the padding, the forward's rule.  fp32 MFMA over the pixel rows, which are cut into chunks of at least 256 rows: the chunks'
 * partial matrices go to the workspace and are added in ascending order; a single chunk writes dwt itself and needs no
 * workspace.  cout <= 256, cin <= 512, b*h*w <= INT_MAX.
 * hf_upconv3x3s2_nhwc_wgrad: x (b,h,w,cin), dz (b,2h,2w,cout) -> dwt (9,cout,cin), dwt[t][co][ci] = sum over (iy,ix) of
 * dz[2 iy - 1 + ky, 2 ix - 1 + kx][co] x[iy,ix][ci] where that output pixel exists.  The same kernel with the stride on the dz side;
 * b*h*w <= INT_MAX / 4.
 * hf_*_wgrad_workspace: the bytes either needs (0 for a single chunk, and 0 outside the contract); HF_EINVAL for a missing or
 * short workspace.
 * hf_maxpool2x2_nhwc_bwd: x as hf_maxpool2x2_nhwc read it (columns [x_col, x_col + c) of rows x_stride wide), dpooled
 * (b,h/2,w/2,c) dense -> columns [dx_col, dx_col + c) of dx's rows, dx_stride wide.  The argmax of every window is recomputed from
 * x with the forward's rule: a strictly greater value or a NaN replaces the maximum, so the first maximum wins a tie.  accumulate =
 * 0: every pixel of the slice is written, dpooled at the argmax, zero elsewhere, zero in a last odd row or column.  accumulate = 1:
 * the same values are added (one fp32 add) to the pixels of whole windows; nothing else is touched. */
int hf_conv3x3s2_nhwc(int b, int h, int w, int cin, int cout, const float *x, const float *wt, const float *scale,
                      const float *shift, int relu, float *y, int y_stride, int y_col, hf_stream_t stream);
size_t hf_conv3x3_nhwc_wgrad_workspace(int b, int h, int w, int cin, int cout);
int hf_conv3x3_nhwc_wgrad(int b, int h, int w, int cin, int cout, const float *x, const float *in_sub, const float *dz,
                          float *dwt, void *workspace, size_t workspace_bytes, hf_stream_t stream);
size_t hf_upconv3x3s2_nhwc_wgrad_workspace(int b, int h, int w, int cin, int cout);
int hf_upconv3x3s2_nhwc_wgrad(int b, int h, int w, int cin, int cout, const float *x, const float *dz, float *dwt,
                              void *workspace, size_t workspace_bytes, hf_stream_t stream);
int hf_maxpool2x2_nhwc_bwd(int b, int h, int w, int c, const float *x, int x_stride, int x_col, const float *dpooled, float *dx,
                           int dx_stride, int dx_col, int accumulate, hf_stream_t stream);
/* The 'concat' fusion of the RPN / RCNN with its path drop (hf/core/models/rpn_model.py:515-546, rcnn_model.py:560-590):
 * out (rows, c1+c2) = [a * masks[0] | b * masks[1]]; masks = two floats ON THE DEVICE (this step's path-drop decision,
 * create_path_drop_masks, rpn_model.py:1130-1193) or NULL for (1, 1).  _grad: grad_a = grad_out[:, :c1] * masks[0],
 * grad_b = grad_out[:, c1:] * masks[1]; either may be NULL. */
int hf_fuse_concat(long long rows, int c1, int c2, const float *a, const float *b, const float *masks, float *out,
                   hf_stream_t stream);
int hf_fuse_concat_grad(long long rows, int c1, int c2, const float *grad_out, const float *masks, float *grad_a,
                        float *grad_b, hf_stream_t stream);
/* The RPN loss (hf/core/models/rpn_model.py:1040-1128 with hf/core/losses.py:131-226) in two passes.  rows = B*P points;
 * seg_logits (rows, k+1); head (rows, k, D), D = 4 nbx + 2 nbt + 4 laid out as _parse_rpn_output slices it (:870-935);
 * label (rows) int32: -1 ignored (the reference's all-zero one-hot row: no segmentation term or gradient, still counted in
 * rows, not foreground), 0 background, 1..k; the targets exactly as hf_bin_box_encode writes them (bin_x / res_x / bin_z / res_z
 * (rows, k), bin_theta / res_theta / res_y (rows), res_size (rows, 3)): the labelled class's entries are picked here
 * (:733-776).  hf_rpn_loss_fwd -> out5 = [segmentation, bin classification, regression, #foreground, total loss]
 * (focal alpha 0.25 gamma 2 on the clipped softmax, x seg_weight / rows; softmax cross-entropy of the three bin groups and
 * smooth-L1 of the true bin's residuals, y and the sizes over foreground points, / max(#fg, 1)).  hf_rpn_loss_bwd -> the
 * gradients w.r.t. seg_logits and head times *upstream (a device scalar; out5 as the forward wrote it); grad_head is
 * zero-filled here.  Limits: k + 1 <= 8, 1 <= nbx, nbt <= 32 (HF_EINVAL beyond).  A label above k and a bin target outside
 * 0..nbx-1 / 0..nbt-1 are the caller's contract: neither is checked.  workspace: hf_rpn_loss_workspace() bytes. */
size_t hf_rpn_loss_workspace(void);
int hf_rpn_loss_fwd(long long rows, int k, int nbx, int nbt, const float *seg_logits, const float *head, const int *label,
                    const int *bin_x, const float *res_x, const int *bin_z, const float *res_z, const int *bin_theta,
                    const float *res_theta, const float *res_y, const float *res_size, float seg_weight, float cls_weight,
                    float reg_weight, float *out5, void *workspace, size_t workspace_bytes, hf_stream_t stream);
int hf_rpn_loss_bwd(long long rows, int k, int nbx, int nbt, const float *seg_logits, const float *head, const int *label,
                    const int *bin_x, const float *res_x, const int *bin_z, const float *res_z, const int *bin_theta,
                    const float *res_theta, const float *res_y, const float *res_size, float seg_weight, float cls_weight,
                    float reg_weight, const float *out5, const float *upstream, float *grad_seg, float *grad_head,
                    hf_stream_t stream);
/* The RCNN loss (hf/core/models/rcnn_model.py:783-810 masks and targets, :1148-1262 loss, hf/core/losses.py:131-200) over
 * `rows` RoIs.  cls_logits (rows, k + 1); head (rows, k, 4 nbx + 2 nbt + 4) laid out as hf_bin_head_decode reads it; iou (rows)
 * the RoI's IoU with its assigned GT; gt_cls (rows) int32 0..k; non_empty (rows) int32 0 / 1; the targets exactly as
 * hf_bin_box_encode writes them for the RoIs (ref_pts = RoI centre, ref_theta = RoI heading) against their GT boxes.
 * Masks, formed here with strict comparisons: cls = (iou < cls_neg_hi or iou > cls_pos_lo) and non-empty, target class 0
 * where iou < cls_neg_hi else gt_cls; reg = iou > reg_pos_lo and non-empty, on the head row / x-z targets of class
 * max(gt_cls - 1, 0) (a row of class 0 never indexes -1).
 * hf_rcnn_loss_fwd -> out6 = [box classification, bin classification, regression, #cls boxes, #reg boxes, total]: softmax
 * cross-entropy summed x cls_weight / #cls; the three bin cross-entropies x cls_weight / #reg; smooth-L1 of the true bin's
 * x / z / theta residuals, y and the three sizes x reg_weight / #reg; a term whose count is 0 is 0.
 * hf_rcnn_loss_bwd -> gradients w.r.t. cls_logits and head times *upstream (a device scalar; out6 as the forward wrote it);
 * grad_head is zero-filled here.  Limits: k + 1 <= 8, 1 <= nbx, nbt <= 32 (HF_EINVAL beyond).  non_empty: any non-zero value
 * is non-empty.  A gt_cls outside 0..k in the cls mask alone is counted in #cls with no term and no gradient; inside the reg
 * mask it is the caller's contract, and so is a bin target outside its bins.  workspace: hf_rcnn_loss_workspace() bytes. */
size_t hf_rcnn_loss_workspace(void);
int hf_rcnn_loss_fwd(long long rows, int k, int nbx, int nbt, const float *cls_logits, const float *head, const float *iou,
                     const int *gt_cls, const int *non_empty, const int *bin_x, const float *res_x, const int *bin_z,
                     const float *res_z, const int *bin_theta, const float *res_theta, const float *res_y, const float *res_size,
                     float cls_neg_hi, float cls_pos_lo, float reg_pos_lo, float cls_weight, float reg_weight, float *out6,
                     void *workspace, size_t workspace_bytes, hf_stream_t stream);
int hf_rcnn_loss_bwd(long long rows, int k, int nbx, int nbt, const float *cls_logits, const float *head, const float *iou,
                     const int *gt_cls, const int *non_empty, const int *bin_x, const float *res_x, const int *bin_z,
                     const float *res_z, const int *bin_theta, const float *res_theta, const float *res_y, const float *res_size,
                     float cls_neg_hi, float cls_pos_lo, float reg_pos_lo, float cls_weight, float reg_weight, const float *out6,
                     const float *upstream, float *grad_cls, float *grad_head, hf_stream_t stream);

/* The RCNN's proposal-target layer (hf/datasets/kitti/kitti_dataset.py:440-770, a host NumPy loop in the reference) on the
 * device.  proposals (b, m, 7) [x, y, z, l, w, h, ry], proposal_count (b) valid rows per frame; gt (b, g, 8)
 * [x, y, z, l, w, h, ry, cls 1..K], gt_count (b).  Outputs (b, R, 7) rois, (b, R) iou_of_rois, (b, R, 8) gt_of_rois and, when
 * stats is not NULL, (b, 4) [#fg, #bg, sampled fg, sampled bg] per frame.
 * IoU: modules.box3d_iou (compute_iou.py:23-64) of every valid (proposal, gt) pair, the BEV overlap of hf_compute_bev_iou.
 * train = 1 (sample_rois_for_rcnn_training, sample_bg_inds :545-680): per RoI max / first argmax over the GTs, per GT the
 *   argmax RoI where its max > 0; fg_thresh = min(reg_pos_lo, cls_pos_lo); fg = RoIs with max >= fg_thresh in ascending
 *   order, then the per-GT argmax RoIs (duplicates kept); easy bg = max < cls_neg_lo; hard bg = cls_neg_lo <= max < cls_neg_hi.
 *   fg and bg: the first min(round(fg_ratio R), #fg) entries of a random permutation of fg, then R - that many bg; fg only:
 *   R fg drawn with replacement; bg only: R bg.  bg slots: int(bg hard_bg_ratio) hard then easy when both exist, else all
 *   from the one that exists, drawn with replacement (floor(u size)).  Output order: fg, then bg.
 *   aug_method (0 none, 1 'single', 2 'multiple', 3 'normal'): aug_roi_by_noise / random_aug_box3d (:690-770) per slot, up
 *   to 10 tries for fg and 1 for bg; each try keeps the RoI with probability 0.2, else draws a box; it stops at IoU >=
 *   fg_thresh with the ASSIGNED gt.  iou_of_rois is that IoU (aug_method 0: the RoI's max IoU).
 * train = 0 (val, :509-513): R must equal m; every proposal with its max IoU and argmax GT row, no sampling.
 * Where the reference fails, this defines:
 *   a frame with no GT (reshape(-1, 0) fails): every RoI is easy bg with IoU 0, gt_of_rois rows are 0, no jitter;
 *   a frame with neither fg nor bg (pdb.set_trace()): R RoIs of the frame drawn with replacement, their max IoU and argmax
 *     GT, no jitter (their IoU lies between every loss mask); stats [0, 0, 0, 0];
 *   proposal_count 0: zero boxes, IoU 0, zero GT rows.
 * Random numbers: a counter hash of (rng_state[0] = base seed, rng_state[1] = call number, frame, slot, draw); the call
 * advances rng_state[1] on the device (a replayed graph draws fresh samples).  rng_state: 2 int64 on the device, required
 * when train = 1, untouched when train = 0.  The draws do not follow NumPy's stream.
 * Limits: b <= 1024, 1 <= m <= 512, g <= 128, 1 <= R <= 512, aug_method 0..3, fg_ratio and hard_bg_ratio in [0, 1],
 * cls_neg_lo <= cls_neg_hi; outside them HF_EINVAL, nothing launched.  workspace: hf_rcnn_targets_workspace(b, m, g) bytes
 * (0 for arguments outside the limits). */
size_t hf_rcnn_targets_workspace(int b, int m, int g);
int hf_rcnn_proposal_targets(int b, int m, int g, const float *proposals, const int *proposal_count, const float *gt,
                             const int *gt_count, float cls_neg_lo, float cls_neg_hi, float cls_pos_lo, float reg_pos_lo,
                             int roi_per_sample, float fg_ratio, float hard_bg_ratio, int aug_method, int train,
                             long long *rng_state, float *rois, float *iou_of_rois, float *gt_of_rois, int *stats,
                             void *workspace, size_t workspace_bytes, hf_stream_t stream);
/* The (b, m, g) 3D IoU of proposals (b, m, 7) x GT (b, g, 8) [x, y, z, l, w, h, ry, cls] (hf/core/box_util.py:131-174
 * proposal_gt_iou3d, written by the RPN's export as proposals_iou): each pair through the device function the target layer
 * samples with, so the values equal hf_rcnn_proposal_targets' IoU bit for bit.  Rows i >= proposal_count[f] and columns
 * j >= gt_count[f] are 0.  Limits as hf_rcnn_proposal_targets: b <= 1024, 1 <= m <= 512, g <= 128. */
int hf_box3d_iou_matrix(int b, int m, int g, const float *proposals, const int *proposal_count, const float *gt,
                        const int *gt_count, float *iou, hf_stream_t stream);
/* The proposal statistics of a validation run (hf/core/evaluator.py:984-1064): compute_iou.box3d_iou_tf, then
 * box_util.compute_recall_iou (hf/core/box_util.py:131-174), per frame.  proposals (b, m, 7), gt (b, g, 8) [box, cls] as
 * hf_box3d_iou_matrix, proposal_count / gt_count (b) the valid rows / columns.  Every valid pair is clipped once; from that
 * BEV overlap come
 *   iou3d (b, m, g), optional (NULL: not written): bit for bit hf_box3d_iou_matrix, zeros in the padding;
 *   iou2d (b, m, g), optional: the BEV IoU, bit for bit hf_compute_bev_iou of the two boxes3d_to_bev rows, zeros in the padding;
 *   best_iou3d, best_iou2d (b, m): the row maxima over the valid GT; best_gt (b, m) int32: the FIRST argmax of the 3D row
 *     (np.argmax: an all-zero row gives 0); 0 / 0 / -1 for rows >= proposal_count and in frames with gt_count 0;
 *   counts (b, 4) int32: proposal_count, gt_count (both clamped to [0, m] / [0, g]), the GT whose column maximum of the 3D IoU
 *     over the valid proposals is > 0.5, the same for > 0.7 (strict, as the reference);
 *   sums (b, 3) fp64: sum of best_iou2d, sum of best_iou3d, sum of |ry of the proposal - ry of gt[best_gt]| (the difference in
 *     fp32), each over the valid proposals, accumulated in fp64 in a fixed order.
 * Deviation from the reference: a frame with gt_count 0 contributes 0 to all three sums; the reference's angle term of such
 * a frame is sum |ry| against an all-zero box.
 * Every output element is written by the call (nothing needs zeroing before); no floating-point atomics: two calls give the
 * same bits.  Two launches: (frame, tile of 256 pairs) workgroups, then one workgroup per frame.  g = 0 is legal with gt NULL.
 * Limits as hf_box3d_iou_matrix: b <= 1024, 1 <= m <= 512, g <= 128; outside them HF_EINVAL, nothing launched.
 * workspace: hf_proposal_stats_workspace(b, m, g) bytes (0 for arguments outside the limits, and when b * g is 0). */
size_t hf_proposal_stats_workspace(int b, int m, int g);
int hf_proposal_stats(int b, int m, int g, const float *proposals, const int *proposal_count, const float *gt,
                      const int *gt_count, float *iou3d, float *iou2d, float *best_iou3d, float *best_iou2d, int *best_gt,
                      int *counts, double *sums, void *workspace, size_t workspace_bytes, hf_stream_t stream);
/* calculate_cls_accuracy (hf/core/evaluator.py:917-932) as counts: logits (rows, c) fp32, target (rows) int32 ->
 * correct (groups) int32, per group of rows / groups consecutive rows the number of rows whose first argmax equals
 * max(target, 0) (a negative target is the reference's all-zero one-hot row, whose argmax is 0).  correct is cleared by the
 * call.  Finite logits are the caller's contract.  Limits: rows >= 0, 2 <= c <= 8, groups >= 1, rows divisible by groups;
 * otherwise HF_EINVAL. */
int hf_argmax_accuracy(long long rows, int c, int groups, const float *logits, const int *target, int *correct,
                       hf_stream_t stream);
/* hf/core/bin_based_box3d_encoder.py:9-139 (tf_decode) for `rows` reference points x k classes: rows = B*p in the RPN
 * (ref_theta NULL = the constant 0), the RoI count in the RCNN.  Per (row, class) inputs are (rows, k[, 3]) arrays;
 * ss / deltas (k,) the per-class XZ search range and bin length; boxes (rows, k, 7) = [x, y, z, l, w, h, ry]. */
int hf_bin_box_decode(long long rows, int k, const float *ref_pts, const float *ref_theta, const int *bin_x,
                      const float *res_x_norm, const int *bin_z, const float *res_z_norm, const int *bin_theta,
                      const float *res_theta_norm, const float *res_y, const float *res_size_norm, const float *mean_sizes,
                      const float *ss, const float *deltas, float r, float delta_theta, float *boxes, hf_stream_t stream);
/* bin_based_box3d_encoder.py:142-269 (tf_encode); rcnn = 0 / 1 selects the rank-3 (RPN) / rank-2 (RCNN) orientation
 * rule.  hi_xz (k,) = float32(2*Ss - 1e-3), hi_theta = float32(2*R - 1e-3), half_delta_theta = float32(0.5*DELTA_THETA):
 * constants the reference forms in Python doubles before TensorFlow casts them. */
int hf_bin_box_encode(long long rows, int k, int rcnn, const float *ref_pts, const float *ref_theta, const float *boxes,
                      const float *mean_sizes, const float *ss, const float *deltas, const float *hi_xz, float r,
                      float hi_theta, float delta_theta, float half_delta_theta, int *bin_x, float *res_x_norm, int *bin_z,
                      float *res_z_norm, int *bin_theta, float *res_theta_norm, float *res_y, float *res_size_norm,
                      hf_stream_t stream);

/* The decoding block of the RPN / RCNN heads in one pass (hf/core/models/rpn_model.py:870-935 parse, :593-605 argmax,
 * :248-290 residual gather, :609-639 mean sizes + tf_decode, :237-246 class gather).  head (rows, k, d) with
 * d = 2*nbx + 2*nbz + 2*nbt + 4 laid out [bin_x logits | res_x_norms | bin_z logits | res_z_norms | bin_theta logits |
 * res_theta_norms | res_y | res_size_norm(3)]; mean_sizes_k (k, 3).  cls == NULL: boxes (rows, k, 7); cls (rows,) int32:
 * boxes (rows, 7), the decoded box of each row's class (rows whose cls is outside [0, k) are left untouched). */
int hf_bin_head_decode(long long rows, int k, int nbx, int nbz, int nbt, const float *head, const float *ref_pts,
                       const float *ref_theta, const float *mean_sizes_k, const float *ss, const float *deltas, float r,
                       float delta_theta, const int *cls, float *boxes, hf_stream_t stream);

/* ------------------------------------------------------------------- PointCNN X-Conv products (callers)
 * hf_xconv_apply       replaces tf.matmul(X, nn_fts_input)  hf/core/feature_extractors/pointcnn.py:133
 *                      x (rows,k,k), f (rows,k,c) -> out (rows,k,c): out[r][i][:] = sum_j x[r][i][j] * f[r][j][:]; k in {4, 8}
 * hf_xconv_apply_grad  its gradients: grad_x (rows,k,k) and / or grad_f (rows,k,c) (either may be NULL)
 * hf_depthwise_k       replaces pf.depthwise_conv2d(.., (1,K)) and the depthwise half of pf.separable_conv2d(.., (1,K))
 *                      on a width-K input (pointfly.py:437-457; pointcnn.py:104-131): x (rows,k,c), w (k,c,m) in
 *                      TensorFlow's depthwise filter layout (1,K,C,M) -> y (rows, c*m), y[r][ch*m+mm] = sum_w x[r][w][ch]*w[w][ch][mm]
 * hf_depthwise_k_grad  grad_x (rows,k,c) and / or grad_w (k,c,m) (zero-filled here, accumulated with atomics)
 * (k, m) supported: k = 8 with m in {1,2,3,4,8}, k = 4 with m in {1,4}; anything else: HF_EINVAL. */
int hf_xconv_apply(long long rows, int k, int c, const float *x, const float *f, float *out, hf_stream_t stream);
int hf_xconv_apply_grad(long long rows, int k, int c, const float *x, const float *f, const float *grad_out, float *grad_x,
                        float *grad_f, hf_stream_t stream);
int hf_depthwise_k(long long rows, int k, int c, int m, const float *x, const float *w, float *y, hf_stream_t stream);
/* hf_xconv_apply followed by hf_depthwise_k in ONE pass (pointcnn.py:133-140): out (rows, c*m) from x (rows,k,k),
 * f (rows,k,c), wd (k,c,m) without the (rows,k,c) product in memory; bit-identical to the two calls.  (k, m): k = 8 with
 * m in 1..4, and (4,1), (4,4), (12,1), (12,2) (the RCNN's layers, rcnn_multiclass.config:157-186).
 * hf_xconv_depthwise_grad: grad_x (rows,k,k), grad_f (rows,k,c), grad_wd (k,c,m; zero-filled here, atomics), any may be NULL. */
int hf_xconv_depthwise(long long rows, int k, int c, int m, const float *x, const float *f, const float *wd, float *out,
                       hf_stream_t stream);
int hf_xconv_depthwise_grad(long long rows, int k, int c, int m, const float *x, const float *f, const float *wd,
                            const float *grad_out, float *grad_x, float *grad_f, float *grad_wd, hf_stream_t stream);
int hf_depthwise_k_grad(long long rows, int k, int c, int m, const float *x, const float *w, const float *grad_y,
                        float *grad_x, float *grad_w, hf_stream_t stream);
/* hf_xconv_depthwise_grad with the row chunks' partial weight gradients written to a workspace (hf_xconv_depthwise_grad_workspace
 * bytes: one row of k c m floats per row chunk) and added in a fixed order, as hf_xconv_depthwise_gather_grad does with its
 * workspace: no atomics, two calls give the same bits of grad_wd; grad_x and grad_f as before.  HF_EWORKSPACE: grad_wd is asked for
 * and the workspace is missing or too small. */
size_t hf_xconv_depthwise_grad_workspace(long long rows, int k, int c, int m);
int hf_xconv_depthwise_grad_ws(long long rows, int k, int c, int m, const float *x, const float *f, const float *wd,
                               const float *grad_out, float *grad_x, float *grad_f, float *grad_wd, void *workspace,
                               size_t workspace_bytes, hf_stream_t stream);
/* the same with a workspace (hf_depthwise_k_grad_workspace bytes): the row chunks' partial weight gradients are written out and
 * added in a fixed order instead of meeting in atomics on the same k*c*m addresses -- deterministic (the row slots of a block
 * meet in a fixed order too: the same bits on every call), and 4x faster for the 8-channel layers of the X-transform where those
 * atomics were the whole cost */
size_t hf_depthwise_k_grad_workspace(long long rows, int k, int c, int m);
int hf_depthwise_k_grad_ws(long long rows, int k, int c, int m, const float *x, const float *w, const float *grad_y, float *grad_x,
                           float *grad_w, void *workspace, size_t workspace_bytes, hf_stream_t stream);
/* The same pass with F_* = [F_delta | gathered features] (pointcnn.py:124-127: tf.gather_nd of the previous layer's features
 * at the neighbour indices, concatenated behind the lifted coordinates) NOT materialised: channels [0, c0) are read from
 * f_delta (rows, k, c0), channels [c0, c0+c1) from the feature table fts (b, n_src, c1) through the neighbour table
 * idx (b, rows_per_cloud, k) (indices into the row's own cloud, as hf_group_point takes them); rows = b * rows_per_cloud.
 * c0 must be a multiple of 64 (it is C/4 of the previous layer in every
 * shipped configuration).  Results are bit-identical to hf_group_point_into + hf_xconv_depthwise on the concatenation.
 * hf_xconv_depthwise_gather_grad: grad_x (rows,k,k), grad_f_delta (rows,k,c0), grad_wd (k,c0+c1,m),
 * grad_fts (b*n_src, c1) -- the last one in gather form through the CSR inverse of the neighbour table (offsets (b, n_src+1),
 * entries (b, rows_per_cloud*k) from hf_index_inverse): every table row is written once, summed in ascending (row, slot) order
 * like hf_group_point_grad_gather; no atomics, no zero fill.  Any gradient may be NULL.  workspace
 * (hf_xconv_depthwise_gather_grad_workspace bytes, may be NULL), laid out as [gathered block's gradient][partial weight
 * gradients]: with it the row chunks' partial depthwise-weight gradients are added in a fixed order instead of meeting in atomics
 * (deterministic grad_wd: the waves of a block add in a fixed order as well, so two calls give the same bits).
 * grad_fts is rebuilt per table row from grad_out (nothing but the table is written), except at
 * the shapes for which xdw_fts_direct (csrc/xconv.hip, a function of the shape alone, with the measurements behind it) picks the
 * staged route: there the gathered block's gradient is written to the first region and summed per table row.  Same values on
 * both routes; on the direct route, and without a workspace, the first region is never touched. */
size_t hf_xconv_depthwise_gather_grad_workspace(int b, int rows_per_cloud, int k, int c0, int c1, int m);
int hf_xconv_depthwise_gather(int b, int n_src, int rows_per_cloud, int k, int c0, int c1, int m, const float *x,
                              const float *f_delta, const float *fts, const int *idx, const float *wd, float *out,
                              hf_stream_t stream);
int hf_xconv_depthwise_gather_grad(int b, int n_src, int rows_per_cloud, int k, int c0, int c1, int m, const float *x,
                                   const float *f_delta, const float *fts, const int *idx, const float *wd,
                                   const float *grad_out, const int *offsets, const int *entries, float *grad_x,
                                   float *grad_f_delta, float *grad_fts, float *grad_wd, void *workspace, size_t workspace_bytes,
                                   hf_stream_t stream);
/* The same pass with the lifting branch's last BatchNorm folded in (csrc/xconv_bn.hip).  On the gather route
 * F_delta = BN1(elu(z1)) is an elementwise function of the second lifting layer's pre-activation z1 (rows, k, c0) and of
 * gamma, beta, mean, invstd (c0 each; the batch statistics hf_lift_elu_bn_fwd / hf_linear_elu_bn_fwd return).  These entries take
 * those five in place of f_delta and rebuild it on load,
 *   a = gamma * invstd;  F_delta = a * (elu(z1) - mean) + beta     (hf_bn_relu_fwd_eval's sequence with mode 2, ELU on exp2),
 * so the normalisation pass and F_delta itself do not exist:
 *   hf_xconv_depthwise_gather_bn(.., z1, gamma, beta, mean, invstd, ..) = hf_xconv_depthwise_gather(.., F_delta, ..), bit for bit.
 * hf_xconv_depthwise_gather_bn_grad: grad_x, grad_fts, grad_wd as hf_xconv_depthwise_gather_grad with a workspace, bit for bit;
 * grad_f (rows, k, c0) is the gradient with respect to F_delta, the BatchNorm's OUTPUT (the same bits again), and with it come the
 * two sums of that BatchNorm's backward pass over the rows x k values of a channel,
 *   dbeta = sum grad_f,   dgamma = sum grad_f * xhat,   xhat = (elu(z1) - mean) * invstd,
 * taken from the values the kernel stores (per lane over its rows, the waves of a block in a fixed order, the blocks in double: no
 * atomics, the same bits on every call; they agree with hf_bn_relu_bwd's to fp32 rounding).  dz1 is then one call of
 * hf_bn_relu_bwd_dx(z1, grad_f, .., dgamma, dbeta, mode 2).  dgamma and dbeta are required with grad_f and untouched without it.
 * workspace (hf_xconv_depthwise_gather_bn_grad_workspace bytes) is required whenever there are rows:
 * [hf_xconv_depthwise_gather_grad's two regions][BatchNorm partial sums: row chunks x 2 x c0].
 * Limits, beyond those of the twins: (k, m) in {(8,1), (8,2), (8,4)}, the gather layers of the shipped PointCNN configurations;
 * rows * k * (c0 + c1) and b * n_src * (c0 + c1) below 2^32 (32-bit element offsets).  Anything else: HF_EINVAL, and the caller
 * keeps hf_bn_relu_fwd_eval + hf_xconv_depthwise_gather. */
size_t hf_xconv_depthwise_gather_bn_grad_workspace(int b, int rows_per_cloud, int k, int c0, int c1, int m);
int hf_xconv_depthwise_gather_bn(int b, int n_src, int rows_per_cloud, int k, int c0, int c1, int m, const float *x,
                                 const float *z1, const float *gamma, const float *beta, const float *mean, const float *invstd,
                                 const float *fts, const int *idx, const float *wd, float *out, hf_stream_t stream);
int hf_xconv_depthwise_gather_bn_grad(int b, int n_src, int rows_per_cloud, int k, int c0, int c1, int m, const float *x,
                                      const float *z1, const float *gamma, const float *beta, const float *mean,
                                      const float *invstd, const float *fts, const int *idx, const float *wd,
                                      const float *grad_out, const int *offsets, const int *entries, float *grad_x,
                                      float *grad_f, float *grad_fts, float *grad_wd, float *dgamma, float *dbeta,
                                      void *workspace, size_t workspace_bytes, hf_stream_t stream);

/* The FIRST layer of a set-abstraction MLP on neighbourhoods read in place: sample_and_group
 * (hf/core/feature_extractors/pointnet_util.py:42-64) materialises new_points (B,M,K,C+3) = [grouped_xyz - centre | points[idx]] and
 * the first tf_util.conv2d (:156-160) reads it back; here the operand rows are assembled from (points, idx, grouped_xyz) while
 * they are staged for the MFMA tiles, so that tensor never exists.  rows = B*M*K, rows_per_cloud = M*K, points (B,n_src,c_feat)
 * (NULL when c_feat == 0), idx (rows) int32, grouped_xyz (rows,3) = query_ball_group's centred coordinates.
 * Column layout of the assembled operand, which `weight` (cout, cin) / `grad_weight` follow:
 *   [feature 0 .. c_feat-1, zeros up to cfp = round_up(c_feat, 4) | x, y, z, 0]      cin = cfp + 4
 * (the caller permutes / pads the layer's weight once per step: a few KB).  Otherwise as hf_linear_bn_fwd / hf_linear_wgrad:
 * z (rows,cout) = operand weight^T + bias with the batch statistics of z from the accumulators; grad_weight = grad_z^T operand. */
int hf_linear_bn_fwd_gather(long long rows, int c_feat, int cout, const float *points, int n_src, long long rows_per_cloud,
                            const int *idx, const float *grouped_xyz, const float *weight, const float *bias, float *z, float eps,
                            float momentum, float *running_mean, float *running_var, float *mean, float *invstd, void *workspace,
                            size_t workspace_bytes, hf_stream_t stream);
int hf_linear_wgrad_gather(long long rows, int cout, int c_feat, const float *grad_z, const float *points, int n_src,
                           long long rows_per_cloud, const int *idx, const float *grouped_xyz, float *grad_weight,
                           void *workspace, size_t workspace_bytes, hf_stream_t stream);

/* The FIRST layer of a feature-propagation MLP on three_nn rows read in place (the FP twin of the block
 * above): pointnet_fp_module (hf/core/feature_extractors/pointnet_util.py:303-329) materialises [interpolated | points1] (B,N,C2+C1)
 * and the first tf_util.conv2d reads it back; here the operand rows are assembled from (points2, idx, weight3, skip) while they
 * are staged for the MFMA tiles, so that tensor never exists -- neither for the forward GEMM nor for the weight gradient.
 * rows = B*N, rows_per_cloud = N, points2 (B,m,c2), idx / weight3 (rows,3) = three_nn's indices (into the row's own cloud; a
 * value outside [0, m) is clamped) and the interpolation weights, skip (rows,c1) = points1, NULL when c1 == 0.
 * Column layout of the assembled operand = the rows of hf_three_interpolate_concat, which `weight` (cout, cin) / `grad_weight`
 * follow (the layer's own weight, zero-padded to cin columns; the padding columns of grad_weight are written as zero):
 *   [ interp 0 .. c2-1 | skip 0 .. c1-1 | zeros up to cin = round_up(c2 + c1, 4) ]
 *   interp j = weight3[r][0] * points2[cloud, idx[r][0], j] + weight3[r][1] * points2[cloud, idx[r][1], j] + weight3[r][2] * ...
 * summed left to right without contraction: the bits hf_three_interpolate_concat writes.  16-byte loads where c2 % 4 == 0 and
 * points2 is 16-byte aligned (for the skip part: c1 % 4 == 0 and skip aligned as well), single columns otherwise.
 * Otherwise as hf_linear_bn_fwd_gather / hf_linear_wgrad_gather: z (rows,cout) = operand weight^T + bias (bias may be NULL) with
 * the batch statistics of z from the accumulators, running_* may be NULL; grad_weight = grad_z^T operand, chunk partials summed
 * in a fixed order; workspaces from hf_linear_bn_fwd_workspace(cout) / hf_linear_wgrad_workspace(rows, cout, cin); nothing
 * allocates or synchronises.  HF_EINVAL, before any device call: rows <= 0, rows % rows_per_cloud != 0, rows >= 2^32,
 * (rows / rows_per_cloud) * m >= 2^31, m < 1, c2 outside 1..1024, c1 outside 0..1024, cout outside 1..256, c1 > 0 without skip,
 * any other required pointer NULL, a workspace that is missing or too small. */
int hf_linear_bn_fwd_interp(long long rows, int c2, int c1, int cout, const float *points2, int m, long long rows_per_cloud,
                            const int *idx, const float *weight3, const float *skip, const float *weight, const float *bias,
                            float *z, float eps, float momentum, float *running_mean, float *running_var, float *mean,
                            float *invstd, void *workspace, size_t workspace_bytes, hf_stream_t stream);
int hf_linear_wgrad_interp(long long rows, int cout, int c2, int c1, const float *grad_z, const float *points2, int m,
                           long long rows_per_cloud, const int *idx, const float *weight3, const float *skip,
                           float *grad_weight, void *workspace, size_t workspace_bytes, hf_stream_t stream);

/* ------------------------------------------------------------------ the optimizer step of the train step */

/* tf.train.AdamOptimizer.apply_gradients over EVERY parameter tensor in one launch (hf/core/trainer.py:71,
 * hf/builders/optimizer_builder.py:59-64; the framework form is one multi-tensor launch per 4 KB of kernel arguments).
 * table: one entry per tensor, ON THE DEVICE; chunk_map: num_chunks pairs (tensor, chunk) of hf_adam_chunk() elements each,
 * on the device; step: one float on the device = the number of THIS step (1 for the first; the caller advances it);
 * grad_scale multiplies every gradient on load (1 / world after a summing all-reduce).
 * mode 0: p -= lr sqrt(1 - b2^t) / (1 - b1^t) * m / (sqrt(v) + eps)   (TensorFlow's placement of epsilon)
 * mode 1: p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)  (torch.optim.Adam's) */
typedef struct hf_adam_entry {
    float *param;
    const float *grad;
    float *exp_avg;
    float *exp_avg_sq;
    long long numel;
} hf_adam_entry;
int hf_adam_chunk(void);
int hf_adam_multi(int num_chunks, const hf_adam_entry *table, const int *chunk_map, const float *step, float lr, float beta1,
                  float beta2, float eps, float grad_scale, int mode, hf_stream_t stream);

/* The reference's train op, slim.learning.create_train_op(..., clip_gradient_norm=1.0) on the averaged gradients
 * (hf/core/trainer.py:68-84) with tf.train.exponential_decay (hf/builders/optimizer_builder.py:102-110), in two launches.
 * hf_adam_sqnorm_partials: one workgroup per row of chunk_map writes partials[row] = sum over its chunk of (grad_scale g)^2 in fp64
 * (partials: num_chunks doubles on the device; a fixed reduction order, no atomics: the same gradients give the same bits).
 * hf_adam_multi_sched: hf_adam_multi's update with
 *   clip_norm > 0: per-tensor tf.clip_by_norm of x = grad_scale g:  x -> (x clip_norm) / max(norm, clip_norm), norm = sqrtf(fp32 of
 *                  the fp64 sum of the tensor's partials in row order).  chunk_map must list a tensor's chunks in consecutive rows,
 *                  in chunk order, and be the map the partials were computed on.  clip_norm == 0: no clipping (partials unused);
 *   decay 0: lr as given; 1: lr decay_factor^((t - 1) / decay_steps); 2 (staircase): lr decay_factor^floor((t - 1) / decay_steps),
 *                  t = *step in fp32 (Adam step t runs at global step t - 1).  The counter is exact up to 2^24 steps.
 * With clip_norm == 0 and decay == 0 the result equals hf_adam_multi's bit for bit.  HF_EINVAL: num_chunks < 0, clip_norm < 0,
 * decay outside 0..2, decay_steps <= 0 or decay_factor <= 0 with decay on, a null pointer that the call needs, hf_adam_multi's
 * checks. */
int hf_adam_sqnorm_partials(int num_chunks, const hf_adam_entry *table, const int *chunk_map, float grad_scale, double *partials,
                            hf_stream_t stream);
int hf_adam_multi_sched(int num_chunks, const hf_adam_entry *table, const int *chunk_map, const float *step, const double *partials,
                        float clip_norm, float lr, int decay, float decay_steps, float decay_factor, float beta1, float beta2, float eps,
                        float grad_scale, int mode, hf_stream_t stream);

/* ------------------------------------------------------------------ feeding a captured step */

/* n (<= hf_copy_multi_max()) device-to-device copies in ONE launch: dst[i] <- src[i], bytes[i] each (the three arrays live on the
 * HOST; they travel in the kernel arguments).  The feed_dict of one sess.run (hf/core/trainer.py:216-226) becomes, for a captured
 * step, the refresh of its static input slots: ~40 tensors per step (points, labels, the neighbour tables of every level) that
 * the framework would copy with one launch each.  Overlapping ranges are not supported. */
int hf_copy_multi_max(void);
int hf_copy_multi(int n, void *const *dst, const void *const *src, const long long *bytes, hf_stream_t stream);

/* ------------------------------------------------------------------ KITTI evaluation (kitti_eval.hip) */

/* The offline KITTI object evaluator, scripts/offline_eval/kitti_native_eval/evaluate_object_3d_offline.cpp (and its _05_iou
 * twin, which differs only in the overlap table), on the device.  All of it is float64.
 *
 * Input: frames in CSR form.  gt_off / det_off (n_frames + 1) int64 are row offsets into gt (n_gt, HF_KITTI_COLS) and
 * det (n_det, HF_KITTI_COLS); pair_off (n_frames + 1) int64 with pair_off[f+1] - pair_off[f] = rows(gt, f) * rows(det, f)
 * numbers the (frame, gt g, det d) pairs as pair_off[f] + g * rows(det, f) + d.  Row columns:
 *   x1 y1 x2 y2 alpha h w l t1 t2 t3 ry extra      extra = truncation (gt) / score (det)
 * gt_type / det_type (int32): HF_KITTI_CAR ... HF_KITTI_OTHER (the caller maps names case-insensitively); gt_occ (int32).
 * Per-frame caps: at most HF_KITTI_MAX_GT gt rows (DontCare included) and HF_KITTI_MAX_DET detections; max_gt / max_det are the
 * caller's largest per-frame counts and must not exceed the caps (HF_EINVAL, nothing launched); offsets that disagree with
 * them are not checked on the device (such frames are left out, and the results are undefined).
 *
 * hf_kitti_eval_overlaps: overlaps (n_pairs, 6) = { image IoU, BEV IoU, 3D IoU, image, BEV, 3D intersection over the
 * detection (criterion 0) } of every pair; the BEV polygons are the reference's toPolygon rectangles, their intersection an
 * fp64 Sutherland-Hodgman clip, the union area(det) + area(gt) - intersection; degenerate rectangles give 0, so do the
 * KITTI DontCare rows (location -1000, dims -1) against a real box.
 *
 * hf_kitti_eval: everything else, on the same inputs.  min_overlap (3,3) float64 ON THE DEVICE = MIN_OVERLAP[metric][class],
 * each in [0, 1); eval_mask bit (metric * 3 + class) = evaluate that pair (the reference evaluates a class for a metric only if
 * one of its detections qualifies; the caller decides); compute_aos = no detection has alpha == -10.  Outputs, indexed
 * [metric (image, BEV, 3D)][class (car, pedestrian, cyclist)][difficulty (easy, moderate, hard)] = list l (27 lists):
 *   thresholds (27, 41) float64, n_thresholds (27) int32  the scores getThresholds selects (<= 41; unused slots 0)
 *   counts (27, 41, 3) int32                             tp, fp (after DontCare suppression), fn summed over frames
 *   precision, aos, aos_ground (27, 41) float64          tp / (tp + fp), similarity / (tp + fp), each replaced by the
 *                                                        maximum over its own and every later slot (std::max_element's
 *                                                        first-largest); aos only for the image metric with compute_aos,
 *                                                        aos_ground (heading, |ry_gt - ry_det|) only for BEV and 3D; else 0
 * Lists outside eval_mask are all zeros.  Every count and the selected thresholds equal the reference's; the similarity sums
 * are added in the reference's order (GT order within a frame, then frames in order), so two calls give the same bits.
 * workspace: hf_kitti_eval_workspace(n_frames, n_gt, n_pairs) bytes (HF_EWORKSPACE if smaller), 256-byte aligned.
 * Scores must not be NaN (the reference sorts them with std::sort). */
#define HF_KITTI_COLS 13
#define HF_KITTI_MAX_GT 128
#define HF_KITTI_MAX_DET 512
#define HF_KITTI_CAR 0
#define HF_KITTI_PEDESTRIAN 1
#define HF_KITTI_CYCLIST 2
#define HF_KITTI_VAN 3
#define HF_KITTI_PERSON_SITTING 4
#define HF_KITTI_DONTCARE 5
#define HF_KITTI_OTHER 6
size_t hf_kitti_eval_workspace(int n_frames, long long n_gt, long long n_pairs);
int hf_kitti_eval_overlaps(int n_frames, const long long *gt_off, const long long *det_off, const long long *pair_off,
                           long long n_gt, long long n_det, long long n_pairs, int max_gt, int max_det, const double *gt,
                           const double *det, double *overlaps, hf_stream_t stream);
int hf_kitti_eval(int n_frames, const long long *gt_off, const long long *det_off, const long long *pair_off, long long n_gt,
                  long long n_det, long long n_pairs, int max_gt, int max_det, const double *gt, const int *gt_type,
                  const int *gt_occ, const double *det, const int *det_type, const double *min_overlap, int eval_mask,
                  int compute_aos, double *thresholds, int *n_thresholds, int *counts, double *precision, double *aos,
                  double *aos_ground, void *workspace, size_t workspace_bytes, hf_stream_t stream);

/* ------------------------------------------------------------------ KITTI result rows (csrc/kitti_result.hip) */

/* The image rectangle and the keep flag of every detection of a batch: the per-box loop of the result writer
 * (hf/core/evaluator_utils.py:88-166, box_3d_projector.project_to_image_space(truncate=True, discard_before_truncation=True)
 * :88-163) in one launch, one thread per detection.  All of it is float64, in the host writer's operation order
 * (inference.project_box3d_to_image, kitti_io.project_to_image).
 * b frames; n detections, flat: boxes3d (n, 7) float32 [x, y, z, l, w, h, ry], scores (n) float32, frame (n) int32 in [0, b);
 * p2 (b, 12) fp64, the ORIGINAL P2 of each frame (float32 values promoted, as the host writer receives them); image_wh (b, 2)
 * int32 the original image size.  Per detection: cos / sin of double(ry), the eight corners of compute_box_corners_3d in its
 * order, [x y z 1] . P2^T, u / w and v / w, the bounding rectangle (a NaN propagates as in np.min / np.max); rejected when the
 * rectangle lies outside the image (x1 > w, y1 > h, x2 < 0, y2 < 0) or is wider than 0.8 w or taller than 0.8 h.
 * Outputs: boxes2d (n, 4) fp64 [x1, y1, x2, y2] truncated to [0, w] x [0, h] (written for every row; zeros for a frame id
 * outside [0, b)); keep (n) uint8 = score >= score_min (fp32 comparison) and not rejected and the frame id is valid.
 * b <= 0 or n < 0, or a NULL pointer with n > 0: HF_EINVAL, nothing launched; n == 0: HF_OK, nothing launched.  No allocation,
 * no synchronisation, no atomics. */
int hf_kitti_result_boxes(int b, long long n, const float *boxes3d, const float *scores, const int *frame, const double *p2,
                          const int *image_wh, float score_min, double *boxes2d, unsigned char *keep, hf_stream_t stream);

/* ------------------------------------------------------------------ RPN training batches (csrc/rpn_batch.hip) */

/* The RPN's training sample (hf/datasets/kitti/kitti_dataset.py:291-440, a host NumPy loop in the reference) for b frames
 * at once.  Random numbers: a counter hash of (rng_state[0] = base seed, rng_state[1] = call number, frame, purpose, index);
 * each call advances rng_state[1] on the device.  rng_state: 2 int64 on the device.  The draws do not follow NumPy's stream;
 * the same rng_state gives bit-identical outputs.  No host synchronisation, no float atomics. */
#define HF_RPN_BATCH_EMPTY 1        /* no point of the frame is in view: its P rows are zeros, src_index -1 */
#define HF_RPN_BATCH_TOO_MANY_FAR 2 /* more than P points at depth >= 40 m: a random P of them, no near point */

/* Points.  points (total, 4) float32 raw velodyne rows [x, y, z, reflectance] of every frame, frame f = rows
 * offsets[f] .. offsets[f+1] (int64, b + 1); velo_to_rect (b, 12) fp64 rows 0..2 of R0_rect . Tr_velo_to_cam (padded 4x4,
 * composed on the host as kitti_io.lidar_to_rect composes it); p2 (b, 12) fp64, the ORIGINAL P2; image_wh (b, 2) int32 the
 * original image size; flip (b) int32.  max_frame_points >= every frame's row count (sizes the grid).
 * View filter (obj_utils.py:221-275), fp64: z > 0, then 0 < u < w and 0 < v < h under P2.  Sampling (:341-371) of the n
 * points in view, near = depth < 40 m: P < n -> every far point and P - n_far near points without replacement; P >= n ->
 * every point once and P - n extra draws, without replacement when P <= 2 n, else with.  Then shuffled.  Flip: x negated.
 * Outputs xyz (b, P, 3) float32 (fp64 rounded once), intensity (b, P, 1) = reflectance - 0.5, src_index (b, P) int32 the
 * frame-local raw row, status (b) int32 HF_RPN_BATCH_* bits.  Limits: b <= 1024, 1 <= P <= 2^20, max_frame_points <= 2^30
 * and <= total.  workspace: hf_rpn_batch_points_workspace(b, total, max_frame_points) bytes (0 outside the limits). */
size_t hf_rpn_batch_points_workspace(int b, long long total, long long max_frame_points);
int hf_rpn_batch_points(int b, int p, long long total, long long max_frame_points, const float *points,
                        const long long *offsets, const double *velo_to_rect, const double *p2, const int *image_wh,
                        const int *flip, long long *rng_state, float *xyz, float *intensity, int *src_index, int *status,
                        void *workspace, size_t workspace_bytes, hf_stream_t stream);

/* Per-point labels, generate_rpn_training_labels (kitti_dataset.py:416-440).  xyz (b, p, 3); boxes (b, g, 7) [x, y, z, l, w,
 * h, ry] (already flipped); classes (b, g) int32 1..K; gt_count (b) valid boxes per frame; expand (0.2, rpn_multiclass.config
 * :265).  Each point walks its frame's boxes in order: inside the box -> that class and that box (a later box overwrites an
 * earlier one); inside exactly one of the box and the box enlarged by l, w, h += 2 expand, y += expand -> class -1 (also
 * overwrites).  label_reg keeps the last box that contained the point (zeros if none).  Inside test: the corner form of
 * obj_utils.is_point_inside (:425-482), strict on every face, fp64.  label_cls (b, p) int32 in {-1, 0..K}, label_reg (b, p, 7).
 * Limits: b <= 1024, 1 <= p <= 2^20, g <= 128. */
int hf_rpn_point_labels(int b, int p, int g, const float *xyz, const float *boxes, const int *classes, const int *gt_count,
                        float expand, int *label_cls, float *label_reg, hf_stream_t stream);

/* Images (kitti_dataset.py:376-400, kitti_aug.py:9-14, 121-202).  images: packed uint8 RGB, HWC per frame at byte
 * image_offsets[f] (int64), size image_wh[f] = (w, h); total_bytes the buffer's size (a frame outside it gives zeros);
 * max_pixels >= every w * h (sizes the grid).  flip (b), jitter (b) int32.  Flip: source column w - 1 - x.  PCA jitter:
 * covariance of x / 255 (np.cov, ddof 1) from exact integer sums, 3x3 Jacobi in fp64 (eigenvalues below 0 taken as 0),
 * noise = (sqrt(e) V) (0.1 N(0, 1)^3), each source value trunc(clip(f64(f32(x) / 255) + noise, 0, 1) * 255).  Resize to
 * (out_h, out_w) with cv2 INTER_LINEAR's geometry (f = (d + 0.5) S / D - 0.5 in fp64 to fp32, s = floor(f), s < 0 -> (0, 0),
 * s >= S - 1 -> (S - 1, 0)), fp32 weights, rounded to nearest: image (b, out_h, out_w, 3) float32 in 0..255.  cv2's fixed-
 * point uint8 path is not restated (bit parity with cv2 is not pinned).  noise (b, 3) fp64 (zeros without jitter);
 * pca_stats (b, 21) fp64 when not NULL: covariance (3x3 row-major), eigenvalues ascending, eigenvectors (3x3, columns).
 * Limits: b <= 1024, w, h, out_h, out_w <= 8192, max_pixels <= 2^23.  workspace: hf_rpn_batch_image_workspace(b, max_pixels). */
size_t hf_rpn_batch_image_workspace(int b, long long max_pixels);
int hf_rpn_batch_image(int b, long long max_pixels, long long total_bytes, const unsigned char *images,
                       const long long *image_offsets, const int *image_wh, const int *flip, const int *jitter, int out_h,
                       int out_w, long long *rng_state, float *image, double *noise, double *pca_stats, void *workspace,
                       size_t workspace_bytes, hf_stream_t stream);

/* ------------------------------------------------------------------ the RPN -> RCNN hand-off (csrc/rcnn_batch.hip) */

/* One (p, 5 + c) float32 row block per frame, [x, y, z, intensity, fg (0.0 / 1.0), rpn_fts...]: the rpn_feature/NAME.npy
 * payload of hf/core/evaluator.py:963-983.  Limits: b <= 1024, 1 <= p <= 2^20, 1 <= c <= 4096; outside them HF_EINVAL,
 * nothing launched. */
#define HF_RCNN_BATCH_BAD_FG 1   /* a fg column value other than 0 or 1 (read as fg = value != 0) */

/* Export side.  xyz (b, p, 3), intensity (b, p, 1), fg_mask (b, p) uint8 / bool (nonzero -> 1.0), rpn_fts (b, p, c) ->
 * rows (b, p, 5 + c); rows 16-byte aligned (float4 stores). */
int hf_rpn_handoff_pack(int b, int p, int c, const float *xyz, const float *intensity, const unsigned char *fg_mask,
                        const float *rpn_fts, float *rows, hf_stream_t stream);
/* Load side, with the flip augmentation (kitti_aug.flip_points).  rows (b, p, 5 + c), flip (b) int32 -> xyz (b, p, 3) with x
 * negated on flipped frames, intensity (b, p, 1), fg_mask (b, p) uint8 (value != 0), rpn_fts (b, p, c) (16-byte aligned),
 * status (b) int32 HF_RCNN_BATCH_* bits (zeroed by the call). */
int hf_rcnn_batch_inputs(int b, int p, int c, const float *rows, const int *flip, float *xyz, float *intensity,
                         unsigned char *fg_mask, float *rpn_fts, int *status, hf_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* HFOPS_H */
