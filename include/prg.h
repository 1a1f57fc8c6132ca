/* prg.h — C-ABI of libprg_hip.so: the MI355X (gfx950) implementation of PointRegGPT's generative data path.
 *
 * The reference (Chen-Suyi/PointRegGPT) has no FFI: this path sits behind plain Python callables.  Each
 * entry point below replaces one of those callables; the reference interface it stands in for is cited as
 *   sd = denoising_diffusion_pytorch/successive_ddnm_diffusion.py      dc = depth_correction_pytorch/depth_correction.py
 * INTEGRATION.md shows the ctypes stub a maintainer of the reference would add to bind them.
 *
 * Conventions
 *   - extern "C", C types only.  Every function returns 0 on success or a negative PRG_E_* code and never
 *     throws or aborts across the boundary; prg_last_error() returns a thread-local message.
 *   - The CALLER owns all tensor memory.  Unless a parameter is documented "host", pointers are DEVICE
 *     pointers (hipMalloc / torch.empty(device='cuda').data_ptr()).  Images are dense row-major float32
 *     (B,1,H,W) exactly as the reference passes them; depth unit: the caller's (the kernels are unit-free).
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream).  Calls are asynchronous with
 *     respect to it and do not synchronise, except *_create / *_destroy / *_reserve.
 *   - The library allocates device memory only inside opaque handles (weights, workspaces, graphs).
 *     Handles are not thread-safe; use one per (process, device).
 */
#ifndef PRG_H
#define PRG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PRG_ABI_VERSION 1

enum {
  PRG_OK = 0,
  PRG_E_INVALID = -1,   /* bad argument (null pointer, size mismatch, unsupported shape) */
  PRG_E_HIP = -2,       /* a HIP runtime call failed; message has hipGetErrorString */
  PRG_E_NOMEM = -3,     /* device allocation failed */
  PRG_E_STATE = -4      /* handle used in the wrong state */
};

/* storage + MFMA input type of a U-Net handle.  PRG_MXFP8 (BASELINE configs[4]): activations stored in bf16, every 3x3
 * convolution with 64-channel-multiple widths runs on v_mfma_scale_f32_32x32x64_f8f6f4 with OCP e4m3 operands and one
 * E8M0 scale per 32 channels (weights quantised at prg_unet_create, activations while they are staged); the rest = bf16. */
/* PRG_F16X3 (round 4): float32 storage and float32 / float64 normalisation arithmetic exactly as PRG_F32, but every
 * convolution contracts on the f16 matrix pipe with both operands split into two f16 halves (a = hi + lo, three MFMAs per
 * product tile, 22-bit operands; csrc/conv_split.hip).  NOT labelled "parity" (that is PRG_F32 alone): its distance from the
 * reference is MEASURED per chain — point-XYZ L-infinity at the end of round 5: 4.5e-6 m (1000-step ancestral @64x64), 3.8e-5 m
 * (250-step DDIM @128x128), 5.3e-5 m (250-step DDIM @256x256, the shipped setting), 7.6e-6 m (the benchmarked 1000-step chain
 * @128x128), all inside the 1e-4 m north star since round 5 (round 4: 1.7e-4 m at 256x256 — the lo halves of unstandardised
 * weights were subnormal f16; the packer now scales each output channel by an exact power of two).  The 256x256 figure is a
 * draw: equal-precision re-orderings of the arithmetic move it within 3.7e-5 .. 8.8e-5 m (the reference's own 1-vs-8-thread
 * spread there is 4.7e-5 m).  tests/test_gpu_f16x3.py asserts these and bench.py's drift_vs_reference re-measures them in every
 * run; 3.9-4.0x PRG_F32's throughput.
 * Operand range: an activation or scaled weight beyond f16's 65504 becomes inf (visible, not silent).                      */
enum { PRG_F32 = 0, PRG_BF16 = 1, PRG_MXFP8 = 2, PRG_F16X3 = 3 };

int prg_abi_version(void);
const char* prg_last_error(void);
/* Name and compute-unit count of the current HIP device (diagnostics; fails loudly when there is none). */
int prg_device_info(char* name, size_t name_len, int* compute_units);

/* ------------------------------------------------------------------------------------------------------
 * Geometry (memory-bound kernels)
 * ---------------------------------------------------------------------------------------------------- */

/* depth2pc_tensor (sd:176-209): depth (B,1,H,W) + K (B,3,3) -> pc (B,H*W,3), valid (B,H*W) as bytes.
 * valid = clip_lo < depth < clip_hi (pass clip_lo > clip_hi to disable clipping, i.e. clip=None);
 * invalid points are filled with `invalid_value` (the reference default is NaN).                          */
int prg_depth2pc(const float* depth, const float* K, float* pc, uint8_t* valid, int B, int H, int W,
                 float clip_lo, float clip_hi, float invalid_value, void* stream);

/* pc2depth_tensor (sd:212-265): z-buffer.  pc (B,N,3), valid (B,N) bytes or NULL (= all valid), K (B,3,3)
 * -> depth (B,1,H,W) nearest z per pixel (0 where nothing lands), mask (B,1,H,W) bytes.
 * Pixel = round-half-even(x*fx/z + cx, y*fy/z + cy); a point counts iff in frame, valid and z > 0.         */
int prg_pc2depth(const float* pc, const uint8_t* valid, const float* K, float* depth, uint8_t* mask,
                 int B, int N, int H, int W, void* stream);

/* Generator.generate's per-scene form (sd:2531-2547): ragged clouds, CSR offsets (B+1, int64, device),
 * each moved by its pose (B,4,4) as p R^T + t (NULL = identity) and z-buffered with its K.
 * `depth_scale` multiplies the stored depth (the reference multiplies by 0.1 right after, sd:2552).          */
int prg_project_points_zbuffer(const float* points, const int64_t* offsets, const float* pose, const float* K,
                               float* depth, uint8_t* mask, int B, int H, int W, float depth_scale,
                               void* stream);

/* Candidate camera poses scored before a chain is spent on one: points / offsets as prg_project_points_zbuffer takes them (ragged
 * float32 clouds, CSR offsets (B+1) int64, DEVICE, offsets[0] may be > 0), poses (B,N,4,4) float32 DEVICE — candidate c of scene
 * b —, K (B,3,3) DEVICE, counts (B,N,3) int32 DEVICE, cleared by the call.  Every row of cloud b is moved by poses[b,c] and
 * projected with prg_project_points_zbuffer's arithmetic (the same fma chain, round-half-even, z > 0 and in-frame test), and
 * counts[b,c] = (in_frame, seen, covered):
 *   in_frame  rows the z-buffer takes;
 *   covered   pixels of that candidate's z-buffer that received a row: the set bytes of prg_project_points_zbuffer's mask for the
 *             same pose;
 *   seen      rows the z-buffer takes whose float32 z <= zmin(pixel) + z_tol (a float32 sum) and, with `box`, whose MOVED
 *             coordinates q satisfy lo <= q <= hi componentwise: the box is applied in the target camera frame, where the
 *             reference crops the target cloud (sd:2641-2650).  Rows that tie for a pixel's nearest depth are all seen.
 * A NaN row fails z > 0 and counts nowhere.  box: 6 floats on the HOST (lo xyz, hi xyz), read during the call, or NULL = no box.
 * Two passes, scatter then count, over per-candidate z-buffers in `workspace` (DEVICE, 4-byte aligned, contents are scratch): it
 * may be smaller than B*N*H*W*4 bytes, the call then works through the candidates in chunks of workspace_bytes / (B*H*W*4), a
 * quotient that must be at least 1.  The counts are integers from atomicMin / atomicAdd on 32-bit words: they depend neither on
 * the order of execution nor on the chunking.  1 <= B, N <= 65535, H, W >= 1, H*W < 2^31, z_tol finite and >= 0; anything else,
 * a null pointer other than box or a workspace that is too small fails with PRG_E_INVALID before any device call.  Asynchronous
 * on `stream`; reads no device data on the host; allocates nothing.
 *
 * prg_pose_candidate_workspace_bytes: B*N*H*W*4 capped at 256 MiB (a whole number of candidates per scene), never less than one
 * candidate per scene; 0 for a size below 1.  Host-only arithmetic: no device call, usable without a GPU; returns the size, not a
 * PRG_E_* code.                                                                                                                 */
size_t prg_pose_candidate_workspace_bytes(int B, int N, int H, int W);
int prg_pose_candidate_counts(const float* points, const int64_t* offsets, const float* poses, const float* K, int B, int N,
                              int H, int W, const float* box, float z_tol, int32_t* counts, void* workspace,
                              size_t workspace_bytes, void* stream);

/* reproject_tensor (sd:268-286) fused: unproject depth*depth_unit, move by pose, z-buffer into the same
 * camera, store z*out_scale.  One kernel, no intermediate point cloud in HBM.                              */
int prg_reproject_zbuffer(const float* depth, const float* K, const float* pose, float* depth_out,
                          uint8_t* mask_out, int B, int H, int W, float depth_unit, float clip_lo,
                          float clip_hi, float out_scale, void* stream);

/* numpy point_cloud + inverse pose (sd:122-143, sd:2627-2628) in float64 like the reference's numpy path:
 * depth (B,1,H,W) float32 * depth_unit -> xyz (B,H*W,3) float64 in the common frame, R^T (p - t), pose NULL =
 * camera frame; rows of invalid pixels are NaN and valid (B,H*W) bytes says which to keep (row-major order
 * is the reference's order after compaction).                                                              */
int prg_unproject_f64(const float* depth, const float* K, const float* pose, double* xyz, uint8_t* valid,
                      int B, int H, int W, float depth_unit, float clip_lo, float clip_hi, void* stream);

/* DepthAugment (dc:577-604): depth (B,1,H,W) -> (B,3,H,W) [depth, 3x3 min over non-zero, difference].   */
int prg_depth_augment(const float* depth, float* out, int B, int H, int W, void* stream);

/* Generator.generate's mask application (sd:2564-2570): keep = prob > thr; depth[~keep] = 0 (in place when
 * depth_out == depth); hit &= keep; img_cond (B,2,H,W) = cat[depth, hit] * 2 - 1 (NULL to skip).
 * `hit` may be NULL (treated as all true, the post-sampling use at sd:2579-2581).                          */
int prg_apply_mask(const float* prob, const float* depth, const uint8_t* hit, float thr, float* depth_out,
                   uint8_t* hit_out, float* img_cond, int B, int H, int W, void* stream);

/* occlusion_filter of Tester.sample (sd:446-463): depth (B,1,H,W) [metres], mask (B,1,H,W) bytes -> out: every pixel
 * more than `threshold` (0.0375) behind the nearest VALID depth of its 3x3 window takes that depth.  out != depth.   */
int prg_occlusion_filter(const float* depth, const uint8_t* mask, float* out, int B, int H, int W, float threshold,
                         void* stream);

/* compute_overlap_ratio of generate_gt.py:68-102 for a batch of cloud pairs, after the caller's voxel down-sampling:
 * pts (total,3) float64 DEVICE, offsets (2*n_pairs+1) int64 DEVICE — pair p is clouds [off[2p],off[2p+1]) and
 * [off[2p+1],off[2p+2]) — counts (n_pairs,2) int32 DEVICE: points of the first / second cloud that have a point of
 * the other strictly within `radius` (float64 squared distances, exact all-pairs test).  max_cloud = largest cloud.  */
int prg_overlap_counts(const double* pts, const int64_t* offsets, int n_pairs, int64_t max_cloud, double radius,
                       int32_t* counts, void* stream);

/* prg_overlap_counts for an indexed list of pairs over a SET of clouds, so that a cloud that is in several pairs is stored (and
 * voxel-gridded by the caller) once: pts (total,3) float64 DEVICE; offsets (n_clouds+1) int64 DEVICE, cloud c is rows
 * [offsets[c], offsets[c+1]), offsets[0] may be > 0; pair_index (n_pairs,2) int32 DEVICE; counts (n_pairs,2) int32 DEVICE.  For
 * (s, t) = pair_index[p]: counts[p] = (rows of cloud s that have a row of cloud t strictly within `radius`, the same from t's
 * side) — prg_overlap_counts' decision: dx*dx + dy*dy + dz*dz in float64 summed left to right, strict < against radius*radius.
 * A cloud may appear in any number of pairs, in either position; s == t is allowed, and then every finite row counts once.  An
 * entry outside [0, n_clouds) makes that pair's counts (-1, -1): the kernel compares the two entries before it forms any address
 * from them, reads no row of pts for such a pair, and no other pair is affected.  max_cloud = largest cloud.  1 <= n_pairs <=
 * 65535, n_clouds >= 1, max_cloud > 0, radius > 0; anything else or a null pointer fails with PRG_E_INVALID before any device
 * call.  counts is cleared by the call itself.  Asynchronous on `stream`; reads no device data on the host; allocates nothing. */
int prg_overlap_counts_indexed(const double* pts, const int64_t* offsets, int n_clouds, const int32_t* pair_index, int n_pairs,
                               int64_t max_cloud, double radius, int32_t* counts, void* stream);

/* Nearest point of the other cloud, for a batch of cloud pairs in the layout of prg_overlap_counts (pts (total,3) float64
 * DEVICE, offsets (2*n_pairs+1) int64 DEVICE, offsets[0] may be > 0; max_cloud = largest cloud, < 2^31): d2 (total) float64
 * and idx (total) int32, DEVICE, one entry per row of pts.  For row i of cloud 2p, d2[i] = the smallest squared distance to a
 * row of cloud 2p+1 — prg_overlap_counts' expression, dx*dx + dy*dy + dz*dz in float64 summed left to right, so the number of
 * d2 < r*r over a cloud is that call's count — and idx[i] = the lowest row of cloud 2p+1, counted from its first row, that
 * attains it; the rows of cloud 2p+1 are answered the same way against cloud 2p by the same call.  Exact all-pairs search:
 * a row starts at +inf / -1 and is replaced on a strict < only, visiting the other cloud in ascending row order, so an empty
 * other cloud, a NaN row (query or candidate: it never wins) and distances that overflow leave +inf / -1.  Rows outside
 * [offsets[0], offsets[2*n_pairs]) are neither read nor written, in pts, d2 or idx.  1 <= n_pairs <= 65535.
 * Asynchronous on `stream`; reads no device data on the host; allocates nothing.                                            */
int prg_nearest_ragged_f64(const double* pts, const int64_t* offsets, int n_pairs, int64_t max_cloud, double* d2,
                           int32_t* idx, void* stream);

/* All pairs within a radius, as a ragged list: the ground-truth correspondences of a batch of cloud pairs, in the layout of
 * prg_overlap_counts (pts (total,3) float64 DEVICE, offsets (2*n_pairs+1) int64 DEVICE, offsets[0] may be > 0).  Pair p is the
 * QUERY cloud A = segment 2p against the CANDIDATE cloud B = segment 2p+1 (one direction: the list of B against A is this one
 * with its columns swapped).  Row i of A and row j of B correspond iff dx*dx + dy*dy + dz*dz < radius*radius with dx = b.x - a.x
 * ... in float64, products written out, summed left to right, strict < — the expression of prg_overlap_counts and
 * prg_nearest_ragged_f64, so on one buffer a row of A has matches iff that call's d2 < radius*radius, and the rows with matches
 * are the first call's count.  Exact all-pairs search; a NaN row never matches; an empty A or B yields nothing.
 * The size of the list is data-dependent, hence two calls; both are asynchronous on `stream`, read no device data on the host
 * and allocate nothing.  1 <= n_pairs <= 65535, 0 < max_cloud < 2^31 (largest cloud), 0 <= total < 2^31, radius finite and > 0;
 * anything else, a null pointer or a workspace that is too small fails with PRG_E_INVALID before any device call.
 *
 * prg_radius_pairs_workspace_bytes: bytes of device workspace pass 1 needs for `total` rows (positive, non-decreasing).
 * Host-only arithmetic: no device call, usable without a GPU; returns the size, not a PRG_E_* code.                          */
size_t prg_radius_pairs_workspace_bytes(int64_t total);

/* Pass 1: per query row the number of matches, then an exclusive scan over buffer rows.  row_start (total+1) int64 DEVICE,
 * written in full: row_start[r] = number of list rows produced by query rows (rows of the even segments) with buffer row < r;
 * rows of odd segments and rows outside [offsets[0], offsets[2*n_pairs]) contribute 0.  row_start[total] is the size of the
 * list, and row_start[offsets[2p]] the first list row of pair p.  workspace: >= prg_radius_pairs_workspace_bytes(total) bytes,
 * DEVICE, 8-byte aligned; contents are scratch.  pts is not written.                                                          */
int prg_radius_count_ragged_f64(const double* pts, const int64_t* offsets, int n_pairs, int64_t total, int64_t max_cloud,
                                double radius, int64_t* row_start, void* workspace, size_t workspace_bytes, void* stream);

/* Pass 2, with pass 1's row_start and the same pts / offsets / n_pairs / max_cloud / radius: corr (capacity,2) int32 DEVICE;
 * the matches of query row r occupy rows [row_start[r], row_start[r+1]) as (i, j) = (row of A counted from A's first row, row
 * of B counted from B's first row), j ascending — so the list is ordered by pair, then i, then j, the same on every run.  A list
 * row whose position is >= capacity is not written (nothing past the buffer, ever): the caller compares row_start[total] with
 * capacity.  capacity == 0 writes nothing (corr may then be NULL).  Rows of pts outside the segments are not read.           */
int prg_radius_fill_ragged_f64(const double* pts, const int64_t* offsets, int n_pairs, int64_t max_cloud, double radius,
                               const int64_t* row_start, int64_t capacity, int32_t* corr, void* stream);

/* Neighbour tables from the list of passes 1 and 2: per query row its `limit` nearest candidates within the radius, nearest
 * first — the K-nearest-within-a-radius tables of a KPConv pyramid (neighbours, sub-sampling, up-sampling).  pts / offsets /
 * n_pairs / max_cloud: the buffer passes 1 and 2 ran on; row_start (total+1) and corr (list_rows,2): their complete output,
 * list_rows = row_start[total].  corr is never read at or beyond list_rows; list_rows == 0 allows corr == NULL.
 * table int32 DEVICE: query row i of pair p owns the `limit` slots from (table_offsets[p] + i) * limit on (table_offsets
 * (n_pairs) int64 DEVICE: the first table row of every pair).  Its matches are ordered by (dx*dx + dy*dy + dz*dz ascending, the
 * expression of passes 1 and 2 recomputed from pts, then j ascending); the first `limit` are written as index_base[p] + j
 * (index_base (n_pairs) int32 DEVICE, NULL = 0), every remaining slot as pad[p] (pad (n_pairs) int32 DEVICE, NULL = the number
 * of rows of the candidate cloud).  Every slot of every query row is written exactly once and nothing else is; pts, row_start
 * and corr are not written.  1 <= n_pairs <= 65535, 0 < max_cloud < 2^31, list_rows >= 0, 1 <= limit <= 1024; anything else or
 * a null pointer fails with PRG_E_INVALID before any device call.  Asynchronous on `stream`; reads no device data on the host;
 * allocates nothing.                                                                                                          */
int prg_radius_select_ragged_f64(const double* pts, const int64_t* offsets, int n_pairs, int64_t max_cloud,
                                 const int64_t* row_start, const int32_t* corr, int64_t list_rows, int limit,
                                 const int64_t* table_offsets, const int32_t* index_base, const int32_t* pad, int32_t* table,
                                 void* stream);

/* Oriented surface normals from neighbour tables: per row the eigenvector of the smallest eigenvalue of its neighbourhood's
 * scatter matrix, turned towards its cloud's viewpoint, and the surface variation lambda_min / (lambda_0 + lambda_1 + lambda_2) —
 * bit for bit `postprocess.estimate_normals`, which states every operation in order (float64, no fma, IEEE / and sqrt: sums
 * over the slots as 8 partial sums, slot s to partial s mod 8, combined by a fixed tree; two passes, mean then scatter matrix;
 * 6 cyclic Jacobi sweeps; the normal is not renormalised).
 * pts (total,3) float64 DEVICE: a stack of C clouds, cloud c = rows [offsets[c], offsets[c+1]) (offsets (C+1) int64 DEVICE).
 * table (Q, limit) int32 DEVICE with indices into the stack and table_offsets (C+1) int64 DEVICE: table row table_offsets[c] + i
 * belongs to row offsets[c] + i of pts — what prg_radius_select_ragged_f64 writes for the self-search of every cloud with
 * index_base = the cloud's first row.  count (Q) int32 DEVICE: the matches of each table row before truncation; the valid slots
 * of a row are its first k = min(count, limit), the others are never read.  pad (C) int32 DEVICE or NULL, select's argument:
 * accepted so that select's arguments pass through unchanged, and not read — validity is by count alone.  A valid slot's index
 * is clamped into the row's own cloud before pts is read (on select's output that changes nothing).  Q: the rows of table, count
 * and of the outputs; table rows outside [table_offsets[0], table_offsets[C]) are neither read nor written.
 * viewpoints (C,3) float64 DEVICE: the normal n of row p is negated iff (nx*(vx-px) + ny*(vy-py)) + nz*(vz-pz) < 0.  A row with
 * k < min_neighbors, or with a non-finite coordinate, gets (0, 0, 1) and variation 0 and is not oriented.
 * normals (Q,3) float64 DEVICE; variation (Q) float64 DEVICE or NULL; scatter (Q,6) float64 DEVICE or NULL — the debug form: the
 * six sums xx, xy, xz, yy, yz, zz before the decomposition, NULL in every product call.  Every element of an owned row is
 * written exactly once by one thread (no atomics, no workspace) and nothing else is; pts, table and count are not written.
 * 1 <= C <= 65535, 0 <= Q < 2^31, 1 <= limit <= 1024, min_neighbors >= 3, no output may be pts; anything else or a null required
 * pointer fails with PRG_E_INVALID before any device call.  Q == 0 returns 0 without a launch (the pointers may then be NULL).
 * Asynchronous on `stream`; reads no device data on the host; allocates nothing.                                               */
int prg_normals_ragged_f64(const double* pts, const int64_t* offsets, int C, const int32_t* table, const int64_t* table_offsets,
                           const int32_t* pad, const int32_t* count, int64_t Q, int limit, const double* viewpoints,
                           int min_neighbors, double* normals, double* variation, double* scatter, void* stream);

/* Node patches: the point-to-node partition of a coarse-to-fine registration network as per-node tables.  d2 (total) float64 and
 * assign (total) int32, DEVICE: the d2 and idx prg_nearest_ragged_f64 wrote for the buffer [points_0 | nodes_0 | points_1 |
 * nodes_1 | ...] with these `offsets` (2*n_pairs+1 int64 DEVICE, offsets[0] may be > 0) — "pair" c is cloud c: segment 2c its
 * points, segment 2c+1 its nodes, so assign[r] of a point row r is its nearest node, counted from the cloud's first node, or -1
 * (a NaN point, no node).  Only the entries of point rows are read; an assign outside [0, nodes of the cloud) counts as -1.
 * table int32 DEVICE: node k of cloud c owns the `limit` slots from (table_offsets[c] + k) * limit on, and sizes[table_offsets[c]
 * + k] (table_offsets (n_pairs) int64 DEVICE: the first table row of every cloud).  The node's members, the points with assign ==
 * k, are ordered by (d2 ascending, then row ascending); the first `limit` are written as index_base[c] + i, i the point's row
 * counted from the cloud's first point (index_base (n_pairs) int32 DEVICE, NULL = 0), every remaining slot as pad[c] (pad
 * (n_pairs) int32 DEVICE, NULL = the number of point rows of the cloud); sizes = the number of members BEFORE truncation, 0 for a
 * node without members.  A node may own any number of points.  Every slot and every size of every node is written, the same
 * bytes on every run (a pad pass, then one writer per slot: no atomics, no sort), and nothing else is; d2 and assign are not
 * written.  The d2 of an assigned row must not be NaN (prg_nearest_ragged_f64 never produces one).  max_cloud / max_nodes: the
 * largest number of points / nodes of a cloud.  1 <= n_pairs <= 65535, 0 < max_cloud < 2^31, 0 < max_nodes < 2^31, 1 <= limit <=
 * 256; anything else or a null pointer fails with PRG_E_INVALID before any device call.  Asynchronous on `stream`; reads no
 * device data on the host; allocates nothing.                                                                                 */
int prg_patch_tables_ragged(const double* d2, const int32_t* assign, const int64_t* offsets, int n_pairs, int64_t max_cloud,
                            int64_t max_nodes, int limit, const int64_t* table_offsets, const int32_t* index_base,
                            const int32_t* pad, int32_t* table, int32_t* sizes, void* stream);

/* Patch against patch: the coarse ground truth of n_pairs items.  pts / offsets: the layout of prg_overlap_counts, segment 2p the
 * fine points of item p's source cloud, segment 2p+1 of its target cloud.  tables (rows, limit) int32 DEVICE: the patch tables of
 * all 2*n_pairs clouds with LOCAL point rows (index_base NULL) and pad = the cloud's rows (pad NULL); table_offsets (2*n_pairs+1)
 * int64 DEVICE: the first table row of every cloud, and the end.  A patch is the entries of its table row inside [0, rows of the
 * cloud); anything else is a pad.  For source node a and target node b of item p, with ms / mt nodes in the two clouds,
 *   hits[2 * (hit_offsets[p] + a * mt + b)]     = points i of patch a that have a point j of patch b with dx*dx + dy*dy + dz*dz <
 *                                                 radius*radius (the expression and the strict < of prg_radius_count_ragged_f64),
 *   hits[2 * (hit_offsets[p] + a * mt + b) + 1] = points j of patch b that have such a point i of patch a
 * (hit_offsets (n_pairs+1) int64 DEVICE, the exclusive sums of ms * mt; hits (total_node_pairs, 2) int32 DEVICE, dense): every
 * node pair of every item is written exactly once, zeros included, the same bytes on every run; a position outside [0,
 * total_node_pairs) is not written.  A NaN point never matches.  max_nodes: the most nodes of a cloud; max_item_pairs: the
 * largest ms * mt of an item.
 * boxes: NULL, or (rows, 6) float64 DEVICE scratch: the call then writes every patch's bounding box there first and skips (writes
 * zeros for) a node pair whose boxes are at least `radius` apart along an axis, the gap taken as fl(lo_b - hi_a) >= radius in
 * float64.  That is exact (rounding is monotonic: every dx*dx of such a pair is >= radius*radius), so hits is the same with and
 * without it.
 * 1 <= n_pairs <= 65535, 0 < max_nodes < 2^31, 1 <= max_item_pairs <= total_node_pairs <= 2^28, 1 <= limit <= 256, radius finite
 * and > 0; anything else or a null pointer (other than boxes) fails with PRG_E_INVALID before any device call.  Asynchronous on
 * `stream`; reads no device data on the host; allocates nothing; pts and tables are not written.                              */
int prg_patch_overlap_ragged_f64(const double* pts, const int64_t* offsets, int n_pairs, const int32_t* tables,
                                 const int64_t* table_offsets, int64_t max_nodes, int limit, double radius,
                                 const int64_t* hit_offsets, int64_t total_node_pairs, int64_t max_item_pairs, double* boxes,
                                 int32_t* hits, void* stream);

/* Fine-level ground truth: the label matrices of n_sel selected patch pairs.  pts (rows, 3) float64 DEVICE: the fine level's
 * stack; table (nodes, limit) int32 DEVICE: every node's patch as rows of that stack — an entry outside [0, rows) is a pad, and
 * the valid slots need not form a prefix; pairs (n_sel, 2) int32 DEVICE: rows of `table` as (a, b) = (source node, target node).
 * labels (n_sel, limit+1, limit+1) uint8 DEVICE, values 0 / 1; with i = table[a][u], j = table[b][v] and K = limit:
 *   labels[s][u][v] = both slots valid and dx*dx + dy*dy + dz*dz < radius*radius, dx = pts[j].x - pts[i].x (the expression and
 *                     the strict < of prg_radius_count_ragged_f64 and prg_patch_overlap_ragged_f64)
 *   labels[s][u][K] = slot u valid and row u holds no match;   labels[s][K][v] = slot v valid and column v holds no match
 *   labels[s][K][K] = 0
 * Validity is by index only: a valid slot that points at a NaN row matches nothing and has its slack label set.  A pair with a
 * or b outside [0, nodes) stands for two empty patches: its matrix is all zero, and nothing of `table` is read for it.  Every
 * byte of labels is written exactly once, the same byte on every run (one writer per byte: no atomics), and nothing else is;
 * pts, table and pairs are not written.
 * 0 <= rows < 2^31 (pts may be NULL only when rows == 0), 1 <= nodes < 2^31, 1 <= limit <= 256, 1 <= n_sel <= 2^24, radius
 * finite and > 0; anything else or another null pointer fails with PRG_E_INVALID before any device call.  Asynchronous on
 * `stream`; reads no device data on the host; allocates nothing.                                                               */
int prg_patch_corr_labels_f64(const double* pts, int64_t rows, const int32_t* table, int64_t nodes, int limit,
                              const int32_t* pairs, int64_t n_sel, double radius, uint8_t* labels, void* stream);

/* Bytes of device workspace prg_voxel_grid_ragged needs for `total` input rows in `B` segments (non-decreasing in both).
 * Host-only arithmetic: no device call, usable without a GPU; this one returns the size, not a PRG_E_* code.            */
size_t prg_voxel_grid_workspace_bytes(int64_t total, int B);

/* PointCloud.voxel_down_sample for B ragged clouds in one call: per segment exactly prg_host_voxel_down_sample (below) —
 * same bits, same output order — i.e. min over the valid rows, org = min - voxel/2, index = floor((p - org)/voxel) in
 * float64, key = (ix*dy + iy)*dz + iz with dy,dz = max index + 1, voxels in ascending key order, each the sum of its rows
 * taken one after the other in input order from the first row, divided by the count.
 * pts (total,3) float64 DEVICE; valid (total) bytes DEVICE or NULL (= all rows); offsets (B+1) int64 DEVICE, ascending,
 * within [0,total].  Rows with valid == 0, and rows outside [offsets[0], offsets[B]), are ignored entirely (they may hold
 * NaN or nothing at all: `total` may be the capacity of a buffer whose tail is unused).  1 <= B <= 65535, total < 2^31.
 * out (>= total rows,3) float64 DEVICE, compact CSR: segment b's voxel means occupy [out_offsets[b], out_offsets[b+1]),
 *   out_offsets[0] = 0; rows of `out` from out_offsets[B] on are not written.  out_offsets (B+1) int64 DEVICE.
 * status (B) int32 DEVICE: 0 ok; 1 a valid row is non-finite; 2 voxel grid too large: dx*dy*dz >= 2^46, the sort key's room
 *   for one segment (this includes the host's "voxel_size is too small" condition, 2^62).  A segment with status != 0
 *   produces 0 rows.  A segment's rows depend on that segment alone: not on B, on its neighbours or on the launch geometry.
 * workspace: >= prg_voxel_grid_workspace_bytes(total, B) bytes, DEVICE, 8-byte aligned; contents are scratch.
 * Asynchronous on `stream`; reads no device data on the host; allocates nothing.  voxel <= 0 fails with PRG_E_INVALID.  */
int prg_voxel_grid_ragged(const double* pts, const uint8_t* valid, const int64_t* offsets, int B, int64_t total,
                          double voxel, double* out, int64_t* out_offsets, int32_t* status, void* workspace,
                          size_t workspace_bytes, void* stream);

/* The input of a scene-memory update (sd:2661-2680) without stream compaction, for prg_voxel_grid_ragged: segment b of
 * `merged` = segment b of the float32 ragged cloud `memory` (memory_rows rows allocated, CSR memory_offsets (B+1) int64
 * DEVICE) widened to float64 with valid = 1, followed by the HW rows of xyz[b] with valid[b] exactly as prg_unproject_f64
 * leaves them (xyz (B,HW,3) float64, valid (B,HW) bytes).  merged (memory_rows + B*HW, 3) float64, merged_valid
 * (memory_rows + B*HW) bytes, merged_offsets (B+1) int64, all DEVICE: merged_offsets[b] = memory_offsets[b] + b*HW.      */
int prg_merge_memory_f64(const float* memory, const int64_t* memory_offsets, int64_t memory_rows, const double* xyz,
                         const uint8_t* valid, int B, int HW, double* merged, uint8_t* merged_valid,
                         int64_t* merged_offsets, void* stream);

/* Rigid move + bounding-box crop of B ragged float64 clouds in one call: what the writer pool (prg_pool_submit_cloud below)
 * does to a cloud before and after its voxel grid, on the device, so that pre-transform -> crop -> prg_voxel_grid_ragged ->
 * post-transform never leaves the GPU.  pts (total,3) float64, valid (total) bytes or NULL (= all rows), offsets (B+1) int64,
 * all DEVICE and meaning exactly what they mean for prg_voxel_grid_ragged; rows outside [offsets[0], offsets[B]) are neither
 * read nor written.  1 <= B <= 65535, total < 2^31.
 * T (B,16) float64 DEVICE, one row-major 4x4 per segment, or NULL (no segment is moved); has_T (B) bytes DEVICE: segment b is
 *   moved iff has_T[b] != 0, NULL = every segment when T is given.  A moved row is x' = x*T[0] + y*T[1] + z*T[2] + T[3]
 *   (y', z' from rows 1, 2), the products summed left to right in float64 without contraction: prg_pool_submit_cloud's
 *   T_pre / T_post bit for bit.  The rows of a segment that is not moved are copied bit for bit (-0.0 stays -0.0, which a
 *   product with an identity matrix would turn into +0.0).
 * lo, hi: 3 doubles each, HOST, read during the call; both NULL = no crop.  With a crop valid_out[i] = valid[i] &&
 *   lo <= p' <= hi on all three axes (inclusive, tested on the moved point, like prg_host_crop_aabb); without one
 *   valid_out[i] = valid[i] (1 when valid is NULL).  The crop flags rows, it does not compact them: prg_voxel_grid_ragged
 *   skips rows whose flag is 0.
 * Rows with valid == 0 may hold NaN or garbage: their valid_out is 0, their `out` row is unspecified, nothing else follows.
 * out (>= offsets[B] rows,3) float64 DEVICE, may be pts itself (one thread owns one row); valid_out (>= offsets[B]) bytes
 *   DEVICE, may be valid itself, may be NULL only when there is no crop.
 * Asynchronous on `stream`; reads no device data on the host; allocates nothing.                                          */
int prg_rigid_crop_ragged_f64(const double* pts, const uint8_t* valid, const int64_t* offsets, int B, int64_t total,
                              const double* T, const uint8_t* has_T, const double* lo, const double* hi, double* out,
                              uint8_t* valid_out, void* stream);

/* The registration loaders' augmentation of C ragged float64 clouds in one call: cut each cloud to a point limit by a keyed
 * random permutation, move it by its rigid transform, add uniform per-point noise.  postprocess.augment_cloud is the numpy
 * definition; the outputs are its bits.
 * pts (total,3) float64, offsets (C+1) int64, both DEVICE: cloud c is rows [offsets[c], offsets[c+1]) (clamped into
 *   [0, total]), n_c rows; rows outside the segments are not read.  1 <= C <= 65535, total and out_total < 2^31.
 * T (C,16) float64 DEVICE or NULL, has_T (C) bytes DEVICE or NULL: exactly prg_rigid_crop_ragged_f64's, the same arithmetic;
 *   a cloud that is not moved is copied, not multiplied.
 * seeds (C) uint64 DEVICE: one Philox4x32-10 key per cloud (k0 = low word).  Row i (local index in its cloud) draws ONE
 *   call, counter {i, draw, 0x6175676D ("augm"), 0}, giving w0..w3.  Its noise depends on (seed, draw, i) only.
 * keys (total) uint32 DEVICE or NULL: the sort key of row i of cloud c is keys[offsets[c] + i], or w0 when keys is NULL.
 * limit: rows kept per cloud, 0 = all.  m_c = min(n_c, limit (if > 0), out_offsets[c+1] - out_offsets[c]).  If m_c == n_c
 *   the rows keep their order: slot i <- row i.  Otherwise rank(i) = #{u : (key_u, u) < (key_i, i)} and row i goes to slot
 *   rank(i) iff rank(i) < m_c: the kept rows arrive in key order, a random permutation cut at m_c.
 * Position of a kept row: the rigid move first, then, iff noise != 0, per axis a: + (u - 0.5) * noise with
 *   u = ((double)w_{1+a} + 0.5) * 2^-32 — u and u - 0.5 are exact, the product is the one rounding; the noise lies strictly
 *   inside (-noise/2, noise/2).  noise must be finite and >= 0.
 * out_offsets (C+1) int64 DEVICE (clamped into [0, out_total]), out (out_total,3) float64 DEVICE, rows (out_total) int32
 *   DEVICE: out[out_offsets[c] + slot] = the position, rows[...] = i.  Slots beyond m_c are not written.  out must not be
 *   pts: the rows are permuted.
 * Asynchronous on `stream`; reads no device data on the host; allocates nothing; no atomics.                              */
int prg_augment_ragged_f64(const double* pts, const int64_t* offsets, int C, int64_t total, const double* T,
                           const uint8_t* has_T, const uint64_t* seeds, uint32_t draw, const uint32_t* keys, int64_t limit,
                           double noise, const int64_t* out_offsets, int64_t out_total, double* out, int32_t* rows,
                           void* stream);

/* ------------------------------------------------------------------------------------------------------
 * U-Nets (MFMA kernels)
 * ---------------------------------------------------------------------------------------------------- */

typedef struct prg_unet prg_unet;

typedef struct prg_unet_config {
  int32_t dim;               /* base width (64) */
  int32_t n_levels;          /* len(dim_mults) (4) */
  int32_t dim_mults[8];      /* (1,2,4,8) */
  int32_t in_channels;       /* Unet 1 ; MaskUnet 3 (DepthAugment is applied inside prg_maskunet_forward) */
  int32_t conditional;       /* 1: time + camera-parameter conditioning (Unet, sd:802) ; 0: MaskUnet (dc:807) */
  int32_t param_cond_dim;    /* 4 */
  int32_t groups;            /* GroupNorm groups (8) */
  int32_t sigmoid_out;       /* 1: final Sigmoid (MaskUnet) */
} prg_unet_config;

/* Number of float32 parameters the config implies (= sum of the reference module's state_dict sizes).    */
int64_t prg_unet_param_count(const prg_unet_config* cfg);

/* weights: HOST pointer to n_floats float32 = every state_dict tensor of the reference module, flattened and
 * concatenated in state_dict order (sd:802-918 / dc:807-869; pointreggpt_amd.weights.param_spec lists it).
 * The library standardises the Block conv weights (sd:601-616, eps 1e-5), repacks everything for its
 * kernels in `dtype` and uploads it.                                                                        */
int prg_unet_create(const prg_unet_config* cfg, const float* weights, int64_t n_floats, int dtype,
                    prg_unet** out);
int prg_unet_destroy(prg_unet* h);
/* SinusoidalPosEmb frequencies (sd:645-657): freqs (HOST, dim/2 float32) = exp(arange(dim/2) * -ln(1e4)/(dim/2-1)).  The
 * reference evaluates this float32 exp with torch on its own device and its outputs depend on that at the 4e-5 level over
 * a 50-step chain (1 ulp of a frequency x t <= 999), so the table is the caller's: pass what torch computes on the host
 * (pointreggpt_amd.unet does).  Default: this host's libm.  Call before creating samplers on the handle.            */
int prg_unet_set_time_freqs(prg_unet* h, const float* freqs, int n);
/* Pre-size the activation workspace for (B, S) so later forwards never allocate.                          */
int prg_unet_reserve(prg_unet* h, int B, int S);

/* Unet.forward (sd:920-964): x (B,1,S,S), time (B,) int64 DEVICE, param_cond (B,4) -> out (B,1,S,S).      */
int prg_unet_forward(prg_unet* h, const float* x, const int64_t* time, const float* param_cond, float* out,
                     int B, int S, void* stream);
/* MaskUnet.forward (dc:871-906): depth (B,1,S,S) -> keep-probability (B,1,S,S).                            */
int prg_maskunet_forward(prg_unet* h, const float* depth, float* prob, int B, int S, void* stream);

/* Debug taps for kernel unit tests: after a forward, copy an internal activation (converted to float32 NCHW)
 * into `out` (device).  Names: "init_conv","down0_block0","down0_attn","down0_out","mid_attn","up0_out",
 * "final_res","augment".  *C,*H,*W receive its shape.  Enabled by prg_unet_set_taps(h, 1).                  */
int prg_unet_set_taps(prg_unet* h, int enable);
int prg_unet_get_tap(prg_unet* h, const char* name, float* out, int64_t out_capacity_floats, int* C, int* H,
                     int* W, void* stream);

/* Kernel unit-test hook: one 3x3 / stride 1 / pad 1 convolution through the library's own dispatch in `dtype` (PRG_BF16
 * or PRG_MXFP8).  x (B,Cin,H,W) float32 DEVICE, w (Cout,Cin,3,3) float32 HOST (used as is: no standardisation), bias
 * (Cout) float32 HOST or NULL, out (B,Cout,H,W) float32 DEVICE (the bf16 result widened).  Synchronises.           */
int prg_debug_conv3x3(const float* x, const float* w, const float* bias, float* out, int B, int Cin, int Cout, int H, int W,
                      int dtype, void* stream);
/* Kernel unit-test hook (round 4): the two convolutions of a ResnetBlock's Block pair (sd:681-697, 731-733) in bf16 mode through
 * the library's own dispatch:  h = conv3x3(x, w1) + b1, its GroupNorm statistics taken in the epilogue;
 * y = conv3x3(SiLU(GroupNorm_groups(h) * gamma + beta), w2) + b2 with the norm in conv2's fused prologue.  h16 = 0: h is stored as
 * bf16; h16 = 1: as f16, prologue in packed f16, f16 MFMA operands in conv2 (PRG_E_INVALID when the shape's kernels do not
 * implement that).  x (B,Cin,H,W) float32 DEVICE; w1 (C,Cin,3,3), w2 (C,C,3,3), b1, b2, gamma, beta (C) float32 HOST, used as
 * they are; out (B,C,H,W) float32 DEVICE.  Cin, C multiples of 64.  Synchronises.                                              */
int prg_debug_block_pair(const float* x, const float* w1, const float* b1, const float* gamma, const float* beta, const float* w2,
                         const float* b2, float* out, int B, int Cin, int C, int H, int W, int groups, int h16, void* stream);
/* The same for Upsample = nn.Upsample(scale_factor 2, nearest) + Conv2d(Cin, Cout, 3, pad 1) (sd:592-594) in bf16:
 * out (B,Cout,2H,2W).  Shapes the 256-pixel kernel covers run as four 2 x 2-tap sub-pixel convolutions of the source image.   */
int prg_debug_upsample_conv3x3(const float* x, const float* w, const float* bias, float* out, int B, int Cin, int Cout, int H,
                               int W, void* stream);
/* The same for Downsample's Conv2d(Cin, Cout, 4, stride 2, pad 1) (sd:596-597) in bf16: w (Cout,Cin,4,4),
 * out (B,Cout,H/2,W/2).                                                                                             */
int prg_debug_conv4x4s2(const float* x, const float* w, const float* bias, float* out, int B, int Cin, int Cout, int H, int W,
                        void* stream);
/* General form for the float32-storage modes (PRG_F32 / PRG_F16X3): K x K kernel (1, 3 or 4), stride 1 or 2, pad = 0 for
 * K = 1 and 1 otherwise; w (Cout,Cin,K,K), out (B,Cout,Ho,Wo) float32.  Also accepts PRG_BF16 / PRG_MXFP8 for K = 3 / 4.  */
int prg_debug_conv(const float* x, const float* w, const float* bias, float* out, int B, int Cin, int Cout, int H, int W,
                   int dtype, int K, int stride, void* stream);
/* nn.Upsample(x2, nearest) + Conv2d(3, pad 1) (sd:592-594) in any storage mode (PRG_F16X3: the sub-pixel form of the split
 * wave-specialised kernel when Cout % 128 == 0; round 5).  out: (B, Cout, 2H, 2W) float32. */
int prg_debug_upsample_conv(const float* x, const float* w, const float* bias, float* out, int B, int Cin, int Cout, int H, int W,
                            int dtype, void* stream);
/* Kernel unit-test hook: an attention core alone on a given to_qkv output.  qkv (B, 384, N) float32 DEVICE in the reference's
 * layout (q | k | v, each 4 heads x 32, head-major), out (B, 128, N) float32 DEVICE; dtype PRG_F32, PRG_BF16 or PRG_F16X3 is the
 * storage the values are converted to first.  linear = 1: the LinearAttention core (sd:755-768; kernel = 0, not PRG_F16X3).
 * linear = 0: the bottleneck core (sd:789-795); kernel = 0 the generic kernel (PRG_F16X3: the float32 one, as the library would
 * run), kernel = 1 the matrix-pipe kernel of the dtype (bf16 MFMA / split-f16 MFMA).  A token count the chosen kernel does not
 * take, PRG_F32 with kernel = 1 and every other bad argument fail with PRG_E_INVALID before any device call.  Synchronises.   */
int prg_debug_attention_core(const float* qkv, float* out, int B, int N, int dtype, int linear, int kernel, void* stream);
/* Kernel unit-test hook: channel LayerNorm with gain (sd:619-628) plus an optional residual on pixel-major rows.  x, residual
 * (or NULL), out (M, C) float32 DEVICE, g (C) float32 HOST; dtype PRG_F32 or PRG_BF16.  C a multiple of 4 (PRG_F32) or 8
 * (PRG_BF16) and of at most 256 such vectors.  Bad arguments fail with PRG_E_INVALID before any device call.  Synchronises.   */
int prg_debug_layernorm(const float* x, const float* g, const float* residual, float* out, int64_t M, int C, int dtype, void* stream);
/* Kernel unit-test hook: out = x + LN_out_g(to_out(LinearAttention(to_qkv(LN_norm_g(x))))) (sd:583-589, 631-639, 737-769) through
 * the fused kernels, on the weights packed as a handle packs them.  x, out (B, C, N) float32 DEVICE; norm_g (C), w_qkv (384, C),
 * w_out (C, 128), b_out (C), out_g (C) float32 HOST, as the state dict holds them.  dtype PRG_BF16: the bf16 kernels (C = 64, 128,
 * 256); shift_mode 1 = the static softmax shifts (PRG_E_INVALID when their bound does not hold for these weights), 0 = measured
 * maxima, -1 = what a handle would choose; psum 1 / 0 = the row sums of p on the matrix pipe or not, -1 = the library's choice.
 * dtype PRG_F16X3: the split-f16 kernels (C = 64, 128; N a multiple of 64); shift_mode and psum must be -1.  *used_static (may be
 * NULL) receives 1 when the static shifts were used.  Bad arguments fail with PRG_E_INVALID before any device call.  Synchronises. */
int prg_debug_linear_attention_block(const float* x, const float* norm_g, const float* w_qkv, const float* w_out, const float* b_out,
                                     const float* out_g, float* out, int B, int C, int N, int dtype, int shift_mode, int psum,
                                     int* used_static, void* stream);
/* Kernel unit-test hook: the fused ResnetBlock tail, out = SiLU(h * A[b] + Bc[b]) + w_res . cat[s0, s1] + b_res (sd:731-734 with
 * the GroupNorm folded into A, Bc), through the bf16 kernel the forward pass launches.  h (B, N, Cout), s0 (B, N, C0),
 * s1 (B, N, C1) float32 DEVICE, pixel-major, converted to bf16 first; A, Bc (B, Cout) float32 DEVICE; w_res (Cout, C0 + C1),
 * b_res (Cout) float32 HOST, packed as a handle packs a res_conv.  head_w (Cout), head_b (1) float32 HOST or both NULL: with them
 * (Cout = 64 only) the network's 1x1 head runs on the tile and out is (B, N) float32 DEVICE (head_sigmoid 1: sigmoid of it);
 * without them out is (B, N, Cout).  in_place 1: the bf16 h buffer is also the kernel's output buffer, as in the forward pass.
 * (C0 + C1, Cout) one of (128, 64), (192, 128), (256, 128), C0 and C1 multiples of 8.  Bad arguments fail with PRG_E_INVALID
 * before any device call.  Synchronises.                                                                                        */
int prg_debug_resblock_tail(const float* h, const float* s0, const float* s1, const float* A, const float* Bc, const float* w_res,
                            const float* b_res, const float* head_w, const float* head_b, float* out, int B, int N, int C0, int C1,
                            int Cout, int head_sigmoid, int in_place, void* stream);

/* Kernel unit-test hook: ONE convolution through the library's own packer and dispatch with the fused options the forward
 * pass sets on it: two sources, statistics of the output, a prologue on the input, a residual in the epilogue.
 *   storage: PRG_CF_STORE_BF16 the launch of a PRG_BF16 handle, as described below.  PRG_CF_STORE_F16X3 / PRG_CF_STORE_F32: the float
 *   launch of a PRG_F16X3 / PRG_F32 handle (the split-f16 kernels / the exact-f32 kernels): x0, x1 and the residual are copied
 *   without rounding, out is the kernel's float32 output, the packer is called with that dtype, and PRG_CF_PRO_FOLD,
 *   PRG_CF_RES_FOLD and PRG_CF_STATS_ACC are PRG_E_INVALID (the forward pass never sets them on a float launch: there are no
 *   fixed-point accumulators in those modes).  Everything else is as below.
 *   Operands: x0 (B,C0,H,W), x1 (B,C1,H,W) float32 DEVICE (x1 NULL exactly when C1 = 0), converted to bf16; w (Cout,C0+C1,K,K),
 *   bias (Cout) float32 HOST; a NULL bias reaches the launch as NULL.  K = 1 (pad 0) or 3 (pad 1), stride 1.  C0, C1, Cout are
 *   multiples of 8; `groups` cuts Cout (and the folded tensor) into multiples of 8 channels.
 *   prologue (K = 3, C1 = 0, a shape whose kernels have one): x <- SiLU(x * a[b][c] + b[b][c]) with PRG_CF_PRO_TABLES pro_a,
 *   pro_b (B,C0) float32 DEVICE, or PRG_CF_PRO_FOLD coefficients folded from fold_acc (B,groups,2) int64 DEVICE fixed-point
 *   (sum * 2^24, sum of squares * 2^20) and fold_p, fold_q (C0) float32 HOST (a = rstd * p, b = q - mean * a).
 *   residual_mode (K = 1): residual (B,Cout,H,W) float32 DEVICE, converted to bf16; PRG_CF_RES_ADD out = conv + residual,
 *   PRG_CF_RES_TABLES out = conv + SiLU(residual * res_a + res_b) with res_a, res_b (B,Cout) float32 DEVICE, PRG_CF_RES_FOLD the
 *   same from fold_acc / fold_p / fold_q (Cout).  in_place 1: the bf16 residual buffer is also the output buffer.
 *   stats (K = 3): PRG_CF_STATS_SLABS asks for per-tile slabs, PRG_CF_STATS_ACC also offers fixed-point accumulators.  A shape
 *   that fuses nothing gets the separate statistics pass (stats_pass = 1).  sums (B,groups,2) float64 HOST: the slabs of an image
 *   group added in slab order, or the accumulators scaled back; acc_raw (B,groups,2) int64 HOST (all zero when the kernel declined
 *   the accumulators); coef_a, coef_b (B,Cout) float32 DEVICE: the GroupNorm coefficient tables the library's next step makes
 *   of them with gamma, beta (Cout) float32 HOST.  nsplit and acc_done are what the conv launch reported.
 *   slabs (optional, with stats): float32 HOST with room for B * PRG_CF_MAX_SLABS * groups * 2 values; receives the raw slabs
 *   [B][nslabs][groups][2] the sums were made of (nslabs = nsplit, or the statistics pass's count); nslabs = 0 and nothing written
 *   when accumulators were used.
 *   family, th, tw, bm, bn: what launch_conv chose (ConvChoice of conv_choose.h: family is a ConvFamily value, th x tw x bn the
 *   tile of the 3x3 families, bm x bn of the implicit-GEMM ones).
 * out (B,Cout,H,W) float32 DEVICE.  Bad arguments fail with PRG_E_INVALID before any device call.  Synchronises.                 */
enum { PRG_CF_PRO_NONE = 0, PRG_CF_PRO_TABLES = 1, PRG_CF_PRO_FOLD = 2 };
enum { PRG_CF_RES_NONE = 0, PRG_CF_RES_ADD = 1, PRG_CF_RES_TABLES = 2, PRG_CF_RES_FOLD = 3 };
enum { PRG_CF_STATS_OFF = 0, PRG_CF_STATS_SLABS = 1, PRG_CF_STATS_ACC = 2 };
enum { PRG_CF_STORE_BF16 = 0, PRG_CF_STORE_F16X3 = 1, PRG_CF_STORE_F32 = 2 };
enum { PRG_CF_MAX_SLABS = 1024 };
typedef struct prg_conv_fused {
  const float* x0;
  const float* x1;
  const float* w;
  const float* bias;
  const float* pro_a;
  const float* pro_b;
  const float* residual;
  const float* res_a;
  const float* res_b;
  const int64_t* fold_acc;
  const float* fold_p;
  const float* fold_q;
  const float* gamma;
  const float* beta;
  float* out;
  double* sums;
  int64_t* acc_raw;
  float* coef_a;
  float* coef_b;
  int32_t B, C0, C1, Cout, H, W, K, groups;
  int32_t prologue, residual_mode, in_place, stats;
  int32_t nsplit, acc_done, stats_pass;   /* out */
  int32_t storage;
  int32_t family, th, tw, bm, bn, nslabs;   /* out */
  float* slabs;
} prg_conv_fused;
int prg_debug_conv_fused(prg_conv_fused* args, void* stream);

/* prg_debug_conv_choice: which kernel launch_conv would run for a convolution, and with what launch geometry: the library's own
 * selection function on plain values.  HOST only, no device call: the CU count and the PRG_* switches are arguments.
 *   query: PRG_CQ_COUNT int32 in the order of the enum below.  dtype = the handle's (PRG_F32 / PRG_F16X3: float storage, PRG_BF16 /
 *   PRG_MXFP8: bf16 storage); then the conv descriptor; `present` = the PRG_CP_* bits of the launch's non-null pointers
 *   (MX = w_mx and w_mx_scale; FOLD_ACC / FOLD_PQ = pro_fold.acc / pro_fold.P and Q); gn_groups; pro_fold's G and cpg; in_f16,
 *   out_f16, mx_pure; num_cus; the twelve switches as PRG_CONV_WS, PRG_CONV_C64, PRG_CONV_W256, PRG_CONV_DOWN_W256,
 *   PRG_CONV_W256MX, PRG_W256_MIN_TILES, PRG_UP2X2, PRG_H16, PRG_MX_PURE, PRG_SPLIT_UP2X2, PRG_SPLIT_P64, PRG_SPLIT_W512.
 *   query2: NULL, or conv2 of a ResnetBlock whose conv1 is `query`: choice[PRG_CC_H16_PAIR] then answers whether the pair runs with
 *   an f16 tensor between them (num_cus and the switches are read from `query`).
 *   choice: PRG_CC_COUNT int32 (family 0 = no kernel takes the request); exec_scale: executed / algorithmic MACs (1 or 4 / 9).
 * Descriptors launch_conv rejects (sizes <= 0, B Hout Wout >= 2^31, C0 / C1 not multiples of the 16-byte vector, CoutPad not a
 * multiple of 64 or below Cout) fail with PRG_E_INVALID.                                                                         */
enum {
  PRG_CQ_DTYPE = 0, PRG_CQ_B, PRG_CQ_HIN, PRG_CQ_WIN, PRG_CQ_C0, PRG_CQ_C1, PRG_CQ_UPS, PRG_CQ_KH, PRG_CQ_KW, PRG_CQ_STRIDE, PRG_CQ_PAD,
  PRG_CQ_HOUT, PRG_CQ_WOUT, PRG_CQ_COUT, PRG_CQ_COUTPAD, PRG_CQ_KCHUNKS, PRG_CQ_PRESENT, PRG_CQ_GN_GROUPS, PRG_CQ_FOLD_G,
  PRG_CQ_FOLD_CPG, PRG_CQ_IN_F16, PRG_CQ_OUT_F16, PRG_CQ_MX_PURE, PRG_CQ_NUM_CUS, PRG_CQ_SWITCHES, PRG_CQ_COUNT = PRG_CQ_SWITCHES + 12
};
enum {
  PRG_CP_BIAS = 1, PRG_CP_RESIDUAL = 2, PRG_CP_RES_A = 4, PRG_CP_PRO_A = 8, PRG_CP_GN_PARTIALS = 16, PRG_CP_GN_ACC = 32, PRG_CP_MX = 64,
  PRG_CP_S2D = 128, PRG_CP_UP = 256, PRG_CP_SPLIT = 512, PRG_CP_UP_SPLIT = 1024, PRG_CP_F16 = 2048, PRG_CP_RES_FOLD_ACC = 4096,
  PRG_CP_FOLD_ACC = 8192, PRG_CP_FOLD_PQ = 16384
};
enum {
  PRG_CC_FAMILY = 0, PRG_CC_TH, PRG_CC_TW, PRG_CC_BM, PRG_CC_BN, PRG_CC_PRO, PRG_CC_MODE, PRG_CC_TILES_X, PRG_CC_TILES_Y, PRG_CC_TILES_N,
  PRG_CC_GRID, PRG_CC_FUSE_STATS, PRG_CC_NSPLIT, PRG_CC_ACC_DONE, PRG_CC_FILL_TABLES, PRG_CC_IS_MX, PRG_CC_SUPPORTS_PROLOGUE,
  PRG_CC_H16_PAIR, PRG_CC_COUNT
};
int prg_debug_conv_choice(const int32_t* query, const int32_t* query2, int32_t* choice, float* exec_scale);

/* Kernel unit-test hooks: the GroupNorm passes and the conditioning kernels of blocks.hip, each alone through the launch function
 * the forward pass calls.  Every tensor is float32 DEVICE (int64 / int32 where said) and is copied or converted into buffers the
 * hook owns; the few HOST arguments are named.  Bad arguments fail with PRG_E_INVALID before any device call.  All synchronise.
 *
 * prg_debug_gn_stats: launch_gn_stats<T> on x (B, C, HW), converted to T = float (PRG_F32) or bf16 (PRG_BF16) in NHWC.  slabs:
 * room for (B, 1024, groups, 2) floats; the first B * nsplit * groups * 2 receive the raw slabs [B][nsplit][groups][2].  *nsplit
 * (HOST) the slab count the launcher chose.  C / vec (vec = 4 / 8) a power of two <= 256, groups <= 64 divides C.              */
int prg_debug_gn_stats(const float* x, float* slabs, int* nsplit, int B, int C, int HW, int groups, int dtype, void* stream);
/* prg_debug_gn_coeff: launch_gn_coeff on the caller's slabs (B, nsplit, groups, 2), gamma, beta (C).  ss_a (ss_a_floats floats, or
 * NULL) is read at b * ss_a_stride + *row * row_stride (+ C for the shift), ss_b (ss_b_floats floats, or NULL, only with ss_a) at
 * b * ss_b_stride; row (HOST int, or NULL) is uploaded to a device int.  A, Bc (B, C).  C <= 1024, groups <= 64, nsplit <= 1024. */
int prg_debug_gn_coeff(const float* slabs, int nsplit, const float* gamma, const float* beta, const float* ss_a, int64_t ss_a_stride,
                       int64_t ss_a_floats, const float* ss_b, int64_t ss_b_stride, int64_t ss_b_floats, const int* row,
                       int64_t row_stride, float* A, float* Bc, int B, int HW, int C, int groups, void* stream);
/* prg_debug_gn_fold (bf16): the consumers of the fixed-point accumulators acc (B, groups, 2) int64 (sum * 2^24, sum of squares * 2^20).
 *   P, Q directly: entries NULL; p, q (C), or (B, C) with pq_per_image 1.
 *   P, Q from launch_cond_fold: entries (HOST, n_entries rows of four int64: ss_off, C, gamma offset, beta offset into flat), flat
 *   (flat_floats), the conditioning rows ss_a / ss_b / row as in prg_debug_gn_coeff (each row ss_total floats wide), pq
 *   (B, ss_total) in and out with pq_stride = ss_total.  The launch is also handed an accumulator array of zero_words + 64 int64
 *   words of the hook's, every byte 0x5a, to clear zero_words of; zero_out (zero_words + 64 int64) receives that array.  P, Q of
 *   the output are those of entry use_entry, whose C is `C`.
 *   output PRG_GF_NONE (cond_fold alone), PRG_GF_TABLES: coef_a, coef_b (B, C) from launch_gn_coeff_acc, PRG_GF_APPLY: out (B, C, HW)
 *   = launch_affine_silu_fold over x (B, C, HW) and an optional residual, converted to bf16; in_place 1: x's bf16 buffer is also
 *   the output buffer.  C a multiple of 8 and <= 1024 for PRG_GF_APPLY.                                                           */
enum { PRG_GF_NONE = 0, PRG_GF_TABLES = 1, PRG_GF_APPLY = 2 };
typedef struct prg_gn_fold {
  const int64_t* acc;
  const float* p;
  const float* q;
  const int64_t* entries;
  const float* flat;
  const float* ss_a;
  const float* ss_b;
  const int32_t* row;
  float* pq;
  int64_t* zero_out;
  const float* x;
  const float* residual;
  float* out;
  float* coef_a;
  float* coef_b;
  int64_t ss_a_stride, ss_a_floats, ss_b_stride, ss_b_floats, row_stride, flat_floats, zero_words;
  int32_t B, C, HW, groups, pq_per_image, n_entries, use_entry, ss_total, output, in_place;
} prg_gn_fold;
int prg_debug_gn_fold(prg_gn_fold* args, void* stream);
/* prg_debug_affine_silu: out = SiLU(x * A[b][c] + Bc[b][c]) + residual through launch_affine_silu<T>; x, residual (or NULL), out
 * (B, C, HW), A, Bc (B, C); dtype PRG_F32 (C a multiple of 4) or PRG_BF16 (of 8).  in_place 1: x's buffer of T is the output's. */
int prg_debug_affine_silu(const float* x, const float* A, const float* Bc, const float* residual, float* out, int B, int C, int HW,
                          int dtype, int in_place, void* stream);
/* prg_debug_linear: launch_linear with every argument of it: x (R, ldx) read at column xoff, W (O, ldw) at column woff, bias (O) or
 * NULL, act_in / act_out 0 none, 1 SiLU, 2 GELU.  y (R, ldy) is copied in, written at columns [ycol, ycol + O), and copied back. */
int prg_debug_linear(const float* x, int ldx, int xoff, const float* W, int ldw, int woff, const float* bias, float* y, int ldy,
                     int ycol, int R, int I, int O, int act_in, int act_out, void* stream);
/* prg_debug_sinusoidal: the sinusoidal embedding of t (R) int64 (wide 1: launch_sinusoidal) or int32 (wide 0:
 * launch_sinusoidal_i32) with the frequency table freqs (dim / 2): out (R, dim) = sin | cos.  dim even, >= 4.                   */
int prg_debug_sinusoidal(const void* t, const float* freqs, float* out, int R, int dim, int wide, void* stream);

/* Host-only hooks into weight preparation (no GPU needed, HOST pointers throughout): what prg_unet_create would upload.
 * Both copy at most capacity_bytes into `out` and write the size of the result to *bytes; out NULL only reports the size.
 *
 * prg_debug_weight_arena: one arena of a handle of `dtype` built from the flat state dict, under the switch settings `options`
 * (PRG_WOPT_* bits, one per PRG_* environment switch read at load time; PRG_WOPT_DEFAULT = the library's defaults).
 * PRG_ARENA_LAYOUT: every offset of the parameter layout as int64 — per conv in traversal order 23 values (Cout, Cin, KH, KW,
 * CoutPad, kchunks, w_off, b_off, w_flat, ws, mx_off, mx_soff, s2d_off, s2d_kchunks, sp_off, sp_kchunks, h16_off, up_off,
 * sp_scale_off, up_sp_scale_off, up_sp_off, conv2, upsample), then per ResnetBlock 7 (cin, cout, ss_off, fw_res, pq1, pq2, cpad),
 * then per attention block 6 (C, fw_qkv, fw_out, kshift, sp_qkv, sp_out).                                                       */
enum { PRG_WOPT_SPLIT_UP2X2 = 1, PRG_WOPT_FUSED_ATTN = 2, PRG_WOPT_LA_KSHIFT = 4, PRG_WOPT_SPLIT_STEM = 8, PRG_WOPT_DEFAULT = 14 };
enum {
  PRG_ARENA_LAYOUT = 0, PRG_ARENA_PACKED, PRG_ARENA_MX, PRG_ARENA_MX_SCALE, PRG_ARENA_H16, PRG_ARENA_SPLIT, PRG_ARENA_SPLIT_SCALE,
  PRG_ARENA_STEM, PRG_ARENA_STEM_FRAG, PRG_ARENA_STEM_SPLIT, PRG_ARENA_STEM_SPLIT_SCALE, PRG_ARENA_FREQS, PRG_ARENA_ATTN_SPLIT,
  PRG_ARENA_PQ_STATIC, PRG_ARENA_COND_ENTRIES, PRG_ARENA_ATTN, PRG_ARENA_KSHIFT, PRG_ARENA_COUNT,
  PRG_ARENA_ALL = -1   /* every arena in this order, each behind its int64 byte count: one build for all of them */
};
int prg_debug_weight_arena(const prg_unet_config* cfg, const float* weights, int64_t n_floats, int dtype, int options, int arena,
                           void* out, int64_t capacity_bytes, int64_t* bytes);
/* prg_debug_pack_conv: one packing of one conv, w (Cout, Cin, K, K) used as it is, as a handle of `dtype` packs it for a conv in
 * the role `role_bits`; empty where the conv has no such packing.  PRG_PACK_S2D_OIHW (K = 4) / PRG_PACK_UP_OIHW (K = 3): the
 * float32 OIHW tensors of the equivalent convolutions, (Cout, 4 Cin, 3, 3) and (4, Cout, Cin, 2, 2).                              */
enum { PRG_ROLE_CONV2 = 1, PRG_ROLE_UPSAMPLE = 2 };
enum {
  PRG_PACK_MAIN = 0, PRG_PACK_S2D, PRG_PACK_UP, PRG_PACK_MX, PRG_PACK_MX_SCALE, PRG_PACK_H16, PRG_PACK_SPLIT, PRG_PACK_SPLIT_SCALE,
  PRG_PACK_UP_SPLIT, PRG_PACK_UP_SPLIT_SCALE, PRG_PACK_S2D_OIHW, PRG_PACK_UP_OIHW
};
int prg_debug_pack_conv(const float* w, int Cout, int Cin, int K, int dtype, int role_bits, int packing, void* out,
                        int64_t capacity_bytes, int64_t* bytes);

/* ------------------------------------------------------------------------------------------------------
 * Sampler: GaussianDiffusion.sample / p_sample_loop / ddim_sample (sd:1283-1409), DDNM replacement included
 * ---------------------------------------------------------------------------------------------------- */

typedef struct prg_sampler prg_sampler;

/* One denoising transition.  With u = Unet(x, t, param_cond):
 *     x0p = (clip_pred & 1) ? clamp(u,-1,1) : u                              (ddim_sample, sd:1199-1201)
 *     eps = (sqrt_recip * x - x0p) / sqrt_recipm1                            (sd:1158-1162; used iff c_eps != 0)
 *     x0  = (known && kept) ? cond_depth : x0p                               (DDNM replacement, sd:1210-1218; kept = true unless
 *           the row has a keep threshold, prg_sampler_set_keep below)
 *     x0  = (clip_pred & 2) ? clamp(x0,-1,1) : x0                            (p_mean_variance, sd:1250-1251: the ancestral
 *           sampler clamps AFTER the replacement; ddim_sample does not, so known pixels > 1 enter the state as they are)
 *     x'  = c_x0 * x0 + c_x * x + c_eps * eps + sigma * noise                (sd:1173-1180,1280 / sd:1369-1373)
 * Ancestral step t: c_x0 = posterior_mean_coef1[t], c_x = coef2[t], c_eps = 0, sigma = exp(0.5 logvar[t])
 * (0 at t = 0).  DDIM pair (t, t'): c_x0 = sqrt(ac[t']), c_x = 0, c_eps = c, sigma = sigma; last pair:
 * c_x0 = 1, everything else 0.  The host (pointreggpt_amd.diffusion) fills this table from the float64
 * schedule exactly as the reference computes it.
 *
 * The above is objective 0 (pred_x0: u IS x0).  With prg_sampler_set_objective below (1 = pred_noise, 2 = pred_v) and the
 * (p[k], q[k]) pair of transition k, only the first line changes:
 *     x0r = objective ? p[k] * x - q[k] * u : u          two float32 products, each rounded, then one subtraction
 *                                                        (sd:1153-1156 / sd:1169-1171)
 *     x0p = (clip_pred & 1) ? clamp(x0r,-1,1) : x0r
 *     eps = objective == 1 ? u : (sqrt_recip * x - x0p) / sqrt_recipm1      pred_noise: the network output itself, NEVER
 *                                                        re-derived after the clamp or the replacement (sd:1195, 1372)
 *     refine row: x' = known ? clamp(x0r,-1,1) : x
 * The replacement, the second clamp, the update and the keep table are as above.                             */
typedef struct prg_step {
  int32_t t;            /* timestep fed to the U-Net */
  int32_t clip_pred;    /* bit 0: clamp the network output before deriving eps (DDIM rows = 1);
                           bit 1: clamp x0 after the DDNM replacement (ancestral rows = 2);
                           bit 2 (= 4, alone): refine row of has_refine_step (sd:1307-1314, 1374-1388):
                                  x' = known ? clamp(u,-1,1) : x, no replacement, coefficients ignored.
                           clamp is torch.clamp: +-Inf becomes +-1 and NaN stays NaN, so a non-finite network
                           output is never turned into a plausible depth */
  float c_x0, c_x, c_eps, sigma;
  float sqrt_recip, sqrt_recipm1;
} prg_step;

/* steps: HOST array of n_steps transitions, executed in order.  The handle owns the state image, the
 * per-step conditioning table and one captured hipGraph of a full transition (U-Net + update) that is
 * replayed n_steps times; the step index lives in device memory so no host sync occurs inside a run.      */
int prg_sampler_create(prg_unet* unet, const prg_step* steps, int n_steps, int B, int S, prg_sampler** out);
int prg_sampler_destroy(prg_sampler* h);
/* 1 (default): replay the captured hipGraph; 0: launch every kernel eagerly (debug / profiling).          */
int prg_sampler_set_graph(prg_sampler* h, int enable);

/* param_cond (B,4); img_cond (B,2,S,S) in [-1,1] or NULL (unconditional: no DDNM replacement);
 * noise: NULL -> on-device Philox4x32-10 keyed per scene by seeds[b] (HOST array of B uint64; results do
 * not depend on batch composition or rank) ; else DEVICE float32 (noise_slabs, B, S, S) in the reference's
 * draw order (sd:1293,1279 / sd:1339,1369): slab 0 is the start image, slab k+1 feeds transition k and is
 * read only where sigma != 0 — both samplers draw nothing on their last transition, so noise_slabs = n_steps
 * suffices; the call fails with PRG_E_INVALID if a transition with sigma != 0 would read past noise_slabs.
 * out (B,1,S,S) = (x_final + 1) * 0.5  (sd:1316).                                                          */
int prg_sampler_run(prg_sampler* h, const float* param_cond, const float* img_cond, const float* noise,
                    int64_t noise_slabs, const uint64_t* seeds, float* out, void* stream);

/* Stochastic DDNM (sd:1075-1094, 1210-1227: ddnm_sampling_dropout / ddnm_dropout_schedule, and denoise(), sd:1411-1427).
 * keep_p: HOST array of n floats, one threshold per transition of the handle (n must equal its n_steps); NULL clears the table
 * (the default: plain DDNM).  The handle owns the device copy.  In a run with an img_cond, transition k with
 *     keep_p[k] <  0 : replaces every known pixel and draws nothing (exactly the run without a table);
 *     keep_p[k] >= 0 : draws one float32 uniform u in [0,1) per pixel and replaces a known pixel iff u > keep_p[k], compared in
 *                      float32 (`uniform_(0,1) > p`, sd:1214-1216).  0 is a threshold like any other: it draws, and drops the
 *                      pixels whose u == 0; the reference draws nothing when its p is 0, so the host passes -1 there.
 * The refine row (clip_pred == 4) ignores the table: no replacement, no draw, the full known mask (sd:1307-1314).            */
int prg_sampler_set_keep(prg_sampler* h, const float* keep_p, int n);
/* Where the uniforms come from.  NULL (default): on-device Philox4x32-10 with the per-scene key of prg_sampler_run's `seeds`
 * (required then, also in a stored-noise run), counter {pixel quad q, k + 1, 0x6B656570, 0} — the normals use 0x70726721 as third
 * word — word i >> 8 times 2^-24 for pixel 4q + i: exact, on the 2^-24 grid of torch's float32 uniform_, 0 included.
 * Else u: DEVICE float32 (slabs, B, S, S), the caller's; slab k feeds transition k and is read only where keep_p[k] >= 0 (other
 * slabs may hold anything); prg_sampler_run fails with PRG_E_INVALID if a drawing transition would read past `slabs`.          */
int prg_sampler_set_keep_draws(prg_sampler* h, const float* u, int64_t slabs);

/* What the network predicts (GaussianDiffusion's `objective`, sd:1194-1208); semantics at prg_step above.
 * objective: 0 = pred_x0 (default; p, q ignored, may be NULL: clears the table), 1 = pred_noise, 2 = pred_v.
 * p, q: HOST arrays of n floats, one pair per transition of the handle (n must equal its n_steps).  The handle owns
 * the device copies.  pred_noise: (sqrt_recip_alphas_cumprod[t], sqrt_recipm1_alphas_cumprod[t]); pred_v:
 * (sqrt_alphas_cumprod[t], sqrt_one_minus_alphas_cumprod[t]).  Independent of the keep table.  May be called between two runs
 * of one handle: the next run uploads the new table and, where the objective itself changed, captures its graph again.
 * Wrong n, an unknown objective or a NULL table with objective != 0 fail with PRG_E_INVALID and leave the handle as it was. */
int prg_sampler_set_objective(prg_sampler* h, int objective, const float* p, const float* q, int n);

/* Kernel unit-test / bandwidth hook (round 6): the transition update above ALONE (sampler_step_kernel: what p_sample / ddim_sample
 * do after model_predictions, sd:1257-1281 / sd:1369-1373) on caller tensors, `reps` launches back to back on `stream`:
 * x (B,HW) DEVICE, updated in place by every launch; u (B,HW) DEVICE = the network output; img_cond (B,2,HW) DEVICE or NULL;
 * seeds (B) DEVICE uint64 Philox keys (launch i draws noise index i + 1); step: HOST, the same row for every launch.
 * *avg_us (HOST, may be NULL) = HIP-event microseconds per launch.  Synchronises.                                            */
int prg_debug_sampler_step(float* x, const float* u, const float* img_cond, const uint64_t* seeds, const prg_step* step, int B,
                           int HW, int reps, float* avg_us, void* stream);
/* The same with a keep threshold on every launch (prg_sampler_set_keep): keep_p as above (< 0: no draw); keep_u DEVICE
 * (reps, B, HW) stored uniforms, launch i reads slab i, or NULL: launch i takes Philox keep draw i + 1 of seeds[b].           */
int prg_debug_sampler_step_keep(float* x, const float* u, const float* img_cond, const uint64_t* seeds, const prg_step* step,
                                float keep_p, const float* keep_u, int B, int HW, int reps, float* avg_us, void* stream);
/* The same with an objective on every launch (prg_sampler_set_objective): the pair (p, q) for every launch, ignored with
 * objective 0, which is prg_debug_sampler_step_keep.                                                                          */
int prg_debug_sampler_step_objective(float* x, const float* u, const float* img_cond, const uint64_t* seeds,
                                     const prg_step* step, int objective, float p, float q, float keep_p,
                                     const float* keep_u, int B, int HW, int reps, float* avg_us, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * Checkpoint validation (csrc/validate.hip): the forward process, the training loss of one network output, and the sums of
 * the depth-correction metrics.  GaussianDiffusion.q_sample / p_losses (sd:1448-1497), MaskTrainer.compute_metrics
 * (dc:1229-1250).  All pointers are DEVICE pointers unless marked HOST.  Streaming kernels, asynchronous on `stream`, no atomics,
 * no host synchronisation, nothing allocated: per-block partials go to the caller's `workspace` of at least
 * prg_validate_workspace_bytes(B, HW) bytes, 16-byte aligned.  Every float32 step written fl(..) is one rounded operation
 * (the library is built with -ffp-contract=off), which is what torch computes.
 *
 * Noise: `noise` (B,HW) float32 stored normals, or NULL; then `seeds` (B) uint64 DEVICE, one Philox4x32-10 key per sample:
 * counter {pixel quad q, draw, 0x76616C64 ("vald"), 0}, four normals per call for pixels 4q .. 4q + 3 by the sampler's
 * Box-Muller arithmetic (the sampler's own streams carry 0x70726721 and 0x6B656570 as third word: no draw is shared with a chain
 * of the same seeds).  Exactly one of noise and seeds is non-NULL; Philox noise needs HW % 4 == 0.  A sample's numbers depend on
 * its own row, seed and coefficients only, never on B or on the other samples of the launch.
 *
 * Summation order of every float64 sum below: fixed, a function of HW alone (stated in csrc/validate.hip and, in numpy, as
 * pointreggpt_amd.validate.ordered_sum).
 *
 * Bad arguments (a NULL pointer where none is allowed, B < 1 or > 65535, HW < 1 or > 2^30, both or neither of noise and seeds,
 * HW % 4 != 0 with Philox noise, an unknown objective or loss type, a workspace that is too small) fail with PRG_E_INVALID
 * before any device call.
 * ---------------------------------------------------------------------------------------------------- */

/* Host-only arithmetic: no device call, usable without a GPU; returns the size (0 for B or HW out of range), not a PRG_E_* code. */
size_t prg_validate_workspace_bytes(int B, int HW);

/* x_t[b][i] = fl(fl(a[b] * x0[b][i]) + fl(s[b] * n[b][i])): two rounded float32 products and one addition (sd:1451-1453).
 * x0, x_t (B,HW) float32; a[b] = sqrt_alphas_cumprod[t_b], s[b] = sqrt_one_minus_alphas_cumprod[t_b], (B) float32, gathered by
 * the host from its float32 buffers like the reference's extract().  noise_out (B,HW) or NULL: the normals n that were used. */
int prg_q_sample(const float* x0, const float* a, const float* s, const float* noise, const uint64_t* seeds, uint32_t draw,
                 int B, int HW, float* x_t, float* noise_out, void* stream);

/* The loss of the network output u (B,HW) without materialising the target (sd:1476-1497).  Per pixel in float32:
 * target = x0 (objective 0, pred_x0), n (1, pred_noise) or fl(fl(a[b] * n) - fl(s[b] * x0)) (2, pred_v; sd:1164-1167);
 * d = fl(u - target); term = |d| (loss_type 0, l1) or fl(d * d) (1, l2).  Per sample: the terms widened to float64 and added in
 * the fixed order; out[b][0] = sum / HW (the unweighted mean), out[b][1] = out[b][0] * (double)w[b], w[b] = loss_weight[t_b].
 * out (B,2) float64.  n is the stored `noise`, or regenerated from (seeds, draw) exactly as prg_q_sample draws it.  A NaN in
 * one sample's input makes that sample's two numbers NaN and touches no other sample's. */
int prg_diffusion_loss(const float* u, const float* x0, const float* noise, const uint64_t* seeds, uint32_t draw, const float* a,
                       const float* s, const float* w, int objective, int loss_type, int B, int HW, void* workspace,
                       size_t workspace_bytes, double* out, void* stream);

/* The sums of compute_metrics.  prob, input, label (B,HW) float32; mask (B,HW) float32 or NULL: then the label mask is
 * (|fl(label - input)| < tol) ? 1 : 0 in float32, PairedDepthDataset's rule (dc:941).  Per pixel: o = prob > threshold,
 * m = mask > threshold (float32 comparisons: NaN and a value exactly at the threshold are false); out = o ? input : 0,
 * lab = m ? label : 0, d = fl(lab - out).  Per sample: counts[b][2 * m + o] (B,4) int64 (the rows of the reference's bincount
 * matrix: label mask major, output mask minor); sums[b] = (sum |d|, sum fl(d * d)) (B,2) float64 in the fixed order. */
int prg_mask_metrics(const float* prob, const float* input, const float* label, const float* mask, float threshold, float tol,
                     int B, int HW, void* workspace, size_t workspace_bytes, int64_t* counts, double* sums, void* stream);

/* Wall-clock free timing hook for bench.py: average duration in milliseconds of the dominant kernel class
 * (implicit-GEMM convolution launches) measured with HIP events on the run's own stream during the last
 * prg_sampler_run when profiling was enabled with prg_sampler_set_profile(h, 1) (forces eager launches).
 * conv_ms = total time inside conv launches, conv_launches = their count, conv_flops = their 2*MAC count. */
int prg_sampler_set_profile(prg_sampler* h, int enable);
int prg_sampler_get_profile(prg_sampler* h, double* conv_ms, int64_t* conv_launches, double* conv_flops,
                            double* total_ms);
/* Algorithmic bytes of the same launches (each input and output element once, plus the weights): what the PMC-measured
 * HBM traffic of bench.py's `roofline.traffic` is compared with. */
int prg_sampler_get_profile_bytes(prg_sampler* h, double* conv_bytes);
/* 2 * MAC count the same launches EXECUTED: equal to conv_flops except for Upsample convs that ran as four 2 x 2-tap sub-pixel
 * convolutions (4 / 9 of the algorithmic count, which stays the reference operator's). */
int prg_sampler_get_profile_executed(prg_sampler* h, double* conv_flops_executed);
/* Per-SHAPE totals of the same launches (round 5; bench.py `roofline.per_kernel`): one row per distinct convolution shape of the
 * profiled run — launches, milliseconds inside them (HIP events), algorithmic and executed 2 * MAC counts.  rows may be null with
 * max_rows = 0 to query the row count; at most max_rows rows are written, *n_rows receives the number available.
 * No reference counterpart (sd: has no profiler on this path): measurement hook like prg_sampler_get_profile. */
typedef struct prg_profile_shape {
  int32_t cin, cout, k, stride, ups, hout, wout;   /* Conv2d(cin, cout, k, stride) on (hout, wout) outputs; ups: after nn.Upsample(x2) */
  int32_t two_source, prologue;                     /* virtual concat of two tensors (skip connection); fused GroupNorm+SiLU on the input */
  int32_t mx;                                       /* 1: the launches ran on MX-fp8 operands (scale-MFMA); occupies the former padding */
  int64_t launches;
  double ms, flops, flops_executed;
} prg_profile_shape;
int prg_sampler_get_profile_shapes(prg_sampler* h, prg_profile_shape* rows, int32_t max_rows, int32_t* n_rows);
/* The same for the per-transition update kernel (x0 / DDNM replace / posterior / noise: HBM-bound, 20 B per pixel). */
int prg_sampler_get_profile_step(prg_sampler* h, double* step_ms, int64_t* step_launches);

/* ------------------------------------------------------------------------------------------------------
 * Host post-processing of the generated views (HOST pointers; plain C++ threads, no device work)
 *
 * Replaces what Generator.generate delegates to open3d / torchvision / cv2 after every batch (sd:2484-2500,
 * 2586-2685): compaction, rigid moves, PointCloud.crop(AxisAlignedBoundingBox), voxel_down_sample, io.write_point_cloud,
 * utils.save_image, cv2.imwrite, np.savetxt.  The pool runs them on worker threads while the GPU samples the next
 * batch.  Semantics = pointreggpt_amd/postprocess.py (Open3D 0.17 as recalled: parity-unpinned).
 * ---------------------------------------------------------------------------------------------------- */

/* pts (n,3) float64 -> out (<= n,3), *n_out; keep lo <= p <= hi (inclusive).                                     */
int prg_host_crop_aabb(const double* pts, int64_t n, const double* lo, const double* hi, double* out, int64_t* n_out);
/* Voxel-grid mean: voxel = floor((p - (min - voxel/2)) / voxel); out (<= n,3) in ascending voxel order.         */
int prg_host_voxel_down_sample(const double* pts, int64_t n, double voxel, double* out, int64_t* n_out);
/* binary_little_endian PLY with `double x y z` vertices (what the example dataloaders read).                    */
int prg_host_write_ply(const char* path, const double* pts, int64_t n);

typedef struct prg_pool prg_pool;
int prg_pool_create(int n_threads, prg_pool** out);
int prg_pool_destroy(prg_pool* p);              /* finishes queued jobs first */
/* Block until every submitted job has finished; returns the first job error (message via prg_last_error).       */
int prg_pool_wait(prg_pool* p, int64_t* jobs_done);
/* One cloud file (inputs are copied; the call returns immediately): xyz (n,3) float64 rows with valid[i] != 0 (NULL =
 * all) -> T_pre (4x4 row-major or NULL) -> crop to [lo,hi] (if crop) -> voxel mean (if voxel > 0) -> T_post -> PLY.
 * sample-000000: (valid, NULL, crop, 0.025, NULL) (sd:2484-2500); sample-000001: (valid, pose0, crop, 0.025,
 * pose0^-1) (sd:2641-2658).                                                                                    */
int prg_pool_submit_cloud(prg_pool* p, const char* path, const double* xyz, int64_t n, const uint8_t* valid,
                          const double* T_pre, int crop, const double* lo, const double* hi, double voxel,
                          const double* T_post);
/* img (H,W) float32 in [0,1]: kind 0 = utils.save_image (8-bit RGB, x*255+0.5 clamped; sd:2588-2612),
 * kind 1 = cv2.imwrite of uint16(img * 1e4) (sd:2618-2620).                                                     */
int prg_pool_submit_image(prg_pool* p, const char* path, const float* img, int H, int W, int kind);
/* np.savetxt(path, values (rows, cols)) with the default "%.18e" format (sd:2462-2467, 2555-2561).              */
int prg_pool_submit_text(prg_pool* p, const char* path, const double* values, int rows, int cols);

#ifdef __cplusplus
}
#endif
#endif /* PRG_H */
