/* prg_cpu.h — C-ABI of libprg_cpu.so: plain C++ / OpenMP twins of the hot path with HOST pointers (SURVEY.md section 8b:
 * "the prg_cpu_* twins").
 *
 * What it is for: BASELINE configs[0] (`generate_dataset.py -start=0 -stop=1 on CPU, 64x64, 50-step DDIM`: the plumbing run
 * that needs no GPU, selected EXPLICITLY with `--device cpu`) and an independent, native second opinion next to the torch
 * oracle.  What it is not: a fallback.  libprg_hip.so never calls it, pointreggpt_amd never routes to it on its own, and the
 * GPU entry points keep failing loudly when there is no HIP device.
 *
 * Same conventions as prg.h (extern "C", status codes, the caller owns every tensor), except that every pointer is a
 * HOST pointer, calls are synchronous, and there is no stream argument.  Arithmetic: float32 with float64 accumulation
 * in the contractions and the normalisation statistics (like the library's fp32 parity mode), IEEE expf / erff / divide;
 * the geometry functions evaluate the reference's float expressions in the reference's order (bit-exact against the
 * fixtures, like their HIP twins).  sd / dc = the reference's successive_ddnm_diffusion.py / depth_correction.py.
 */
#ifndef PRG_CPU_H
#define PRG_CPU_H

#include "prg.h"

#ifdef __cplusplus
extern "C" {
#endif

const char* prg_cpu_last_error(void);

/* ---- geometry: twins of prg_depth2pc / prg_pc2depth / prg_project_points_zbuffer / prg_reproject_zbuffer /
 *      prg_unproject_f64 / prg_depth_augment / prg_apply_mask (same arguments without the stream) ---- */
int prg_cpu_depth2pc(const float* depth, const float* K, float* pc, uint8_t* valid, int B, int H, int W, float clip_lo,
                     float clip_hi, float invalid_value);                                              /* sd:176-209 */
int prg_cpu_pc2depth(const float* pc, const uint8_t* valid, const float* K, float* depth, uint8_t* mask, int B, int N,
                     int H, int W);                                                                    /* sd:212-265 */
int prg_cpu_project_points_zbuffer(const float* points, const int64_t* offsets, const float* pose, const float* K,
                                   float* depth, uint8_t* mask, int B, int H, int W, float depth_scale);   /* sd:2531-2552 */
/* twin of prg_pose_candidate_counts (prg.h), the bit-exact comparator of its kernels: the same arguments with HOST pointers, no
 * workspace and no stream; one z-buffer per (scene, candidate) at a time.  counts (B,N,3) = (in_frame, seen, covered).           */
int prg_cpu_pose_candidate_counts(const float* points, const int64_t* offsets, const float* poses, const float* K, int B, int N,
                                  int H, int W, const float* box, float z_tol, int32_t* counts);
int prg_cpu_reproject_zbuffer(const float* depth, const float* K, const float* pose, float* depth_out, uint8_t* mask_out,
                              int B, int H, int W, float depth_unit, float clip_lo, float clip_hi, float out_scale);  /* sd:268-286 */
int prg_cpu_unproject_f64(const float* depth, const float* K, const float* pose, double* xyz, uint8_t* valid, int B, int H,
                          int W, float depth_unit, float clip_lo, float clip_hi);                      /* sd:122-143, 2627-2628 */
int prg_cpu_depth_augment(const float* depth, float* out, int B, int H, int W);                         /* dc:577-604 */
int prg_cpu_apply_mask(const float* prob, const float* depth, const uint8_t* hit, float thr, float* depth_out,
                       uint8_t* hit_out, float* img_cond, int B, int H, int W);                        /* sd:2564-2570 */

/* ---- U-Nets: twins of prg_unet_create / _destroy / _set_time_freqs / prg_unet_forward / prg_maskunet_forward ---- */
typedef struct prg_cpu_unet prg_cpu_unet;
int prg_cpu_unet_create(const prg_unet_config* cfg, const float* weights, int64_t n_floats, prg_cpu_unet** out);
int prg_cpu_unet_destroy(prg_cpu_unet* h);
int prg_cpu_unet_set_time_freqs(prg_cpu_unet* h, const float* freqs, int n);
int prg_cpu_unet_forward(prg_cpu_unet* h, const float* x, const int64_t* time, const float* param_cond, float* out, int B,
                         int S);                                                                       /* sd:920-964 */
int prg_cpu_maskunet_forward(prg_cpu_unet* h, const float* depth, float* prob, int B, int S);           /* dc:871-906 */

/* ---- sampler: twin of prg_sampler_create + prg_sampler_run in one call (no graph to keep) ----
 * steps: the prg_step table (n_steps rows); noise: stored draws (noise_slabs, B, S*S) in the reference's order, or NULL ->
 * Philox4x32-10 keyed by seeds[B] (the device generator's counter layout; libm's logf / sincosf, so not bit-identical to
 * the device's draws).  img_cond (B,2,S,S) or NULL.  out (B,1,S,S) in [0,1] (or beyond: ddim_sample does not clamp the
 * replaced pixels).  sd:1283-1409.                                                                                      */
int prg_cpu_sampler_run(prg_cpu_unet* h, const prg_step* steps, int n_steps, const float* param_cond, const float* img_cond,
                        const float* noise, int64_t noise_slabs, const uint64_t* seeds, float* out, int B, int S);
/* The same with the stochastic DDNM keep table of prg_sampler_set_keep / prg_sampler_set_keep_draws (prg.h): keep_p (n_steps)
 * thresholds or NULL; keep_u stored uniforms (keep_slabs, B, S*S), slab k for transition k, read only where keep_p[k] >= 0, or
 * NULL -> Philox with the device's counter layout and its exact 24-bit uniform (bit-identical masks; needs seeds).
 * sd:1075-1094, 1210-1227, 1411-1427.                                                                                     */
int prg_cpu_sampler_run_keep(prg_cpu_unet* h, const prg_step* steps, int n_steps, const float* param_cond, const float* img_cond,
                             const float* noise, int64_t noise_slabs, const uint64_t* seeds, const float* keep_p,
                             const float* keep_u, int64_t keep_slabs, float* out, int B, int S);
/* The same with the objective of prg_sampler_set_objective (prg.h): objective 0 = pred_x0 (p, q ignored, may be NULL), 1 =
 * pred_noise, 2 = pred_v; p, q (n_steps) the per-transition pairs.  The two entries above are this one with objective 0.
 * sd:1153-1171, 1194-1208.                                                                                                */
int prg_cpu_sampler_run_objective(prg_cpu_unet* h, const prg_step* steps, int n_steps, const float* param_cond,
                                  const float* img_cond, const float* noise, int64_t noise_slabs, const uint64_t* seeds,
                                  const float* keep_p, const float* keep_u, int64_t keep_slabs, int objective, const float* p,
                                  const float* q, float* out, int B, int S);

/* ---- conv3x3_c64_kernel's step schedule (pointreggpt_amd/csrc/c64_schedule.h, shared with the kernel) as event rows ----
 * One role's instruction stream in program order: role 0 = producer waves, 1 = consumer waves; depth = halo register sets (2 or
 * 3).  Row = 6 int32 {role, kind (0 issue loads, 1 write LDS, 2 read LDS, 3 barrier), halo, register set, LDS buffer, tile
 * step}, -1 where a field does not apply.  capacity = 0 only counts.  tests/test_c64_schedule.py proves the barrier counts and
 * the buffer / register lifetimes from these rows for every step count before a kernel built on them is launched.           */
int prg_cpu_c64_schedule(int nsteps, int depth, int role, int32_t* events, int64_t capacity, int64_t* n_events);

#ifdef __cplusplus
}
#endif
#endif
