// c64_schedule.h — the step schedule of conv3x3_c64_kernel (conv_c64.hip), in plain integer functions that the kernel and the
// CPU twin library (cpu_ref.cpp: prg_cpu_c64_schedule, tests/test_c64_schedule.py) share.  No HIP type appears here.
//
// A workgroup has two wave classes that meet at workgroup barriers only.  With `depth` halo register sets (2 or 3):
//
//   PRODUCERS  prologue: issue halos 0 .. depth-2 (halo h into register set h % depth), write halo 0 to LDS, issue halo
//              depth-1, barrier;
//              step s = 0 .. padded-1: issue halo s + depth into the set halo s left when it was written, write halo s + 1
//              (issued depth - 1 steps earlier) into LDS buffer (s + 1) & 1, barrier;
//              one closing barrier.
//   CONSUMERS  barrier; step s = 0 .. nsteps-1: read halo s from LDS buffer s & 1, barrier; padded - nsteps padding barriers;
//              one closing barrier.
//
// `padded` is nsteps rounded up to a multiple of depth: the register set of a halo is a compile-time choice, so the producers'
// loop body covers `depth` steps.  A halo index past nsteps - 1 is a clamped reload of the last tile that nobody reads.
//
// The kernel runs depth 2.  Depth 3 (loads two steps ahead) is proved here as well: it was built on this schedule, ran correctly and
// was measured slower (profiles/c64_pipeline_stamps_and_variants.txt), so whoever retries it starts from a schedule that is known good.
#pragma once

#if defined(__HIP__) || defined(__CUDACC__)
#define C64_HD __host__ __device__ inline
#else
#define C64_HD inline
#endif

namespace prg {

C64_HD constexpr int c64_padded_steps(int nsteps, int depth) { return (nsteps + depth - 1) / depth * depth; }
C64_HD constexpr int c64_reg_set(int halo, int depth) { return halo % depth; }
C64_HD constexpr int c64_lds_buf(int halo) { return halo & 1; }
C64_HD constexpr int c64_issued_in_step(int step, int depth) { return step + depth; }   // the halo whose loads step `step` issues
C64_HD constexpr int c64_written_in_step(int step) { return step + 1; }                 // the halo step `step` writes to LDS
C64_HD constexpr int c64_tile_of_halo(int halo, int nsteps) { return halo < nsteps ? halo : nsteps - 1; }   // clamped reloads
C64_HD constexpr int c64_consumer_pad_barriers(int nsteps, int depth) { return c64_padded_steps(nsteps, depth) - nsteps; }
C64_HD constexpr int c64_producer_barriers(int nsteps, int depth) { return 1 + c64_padded_steps(nsteps, depth) + 1; }
C64_HD constexpr int c64_consumer_barriers(int nsteps, int depth) { return 1 + nsteps + c64_consumer_pad_barriers(nsteps, depth) + 1; }

// The two instruction streams as event rows {role, kind, halo, register set, LDS buffer, tile step}; -1 = not applicable.
enum { C64_PRODUCER = 0, C64_CONSUMER = 1 };
enum { C64_ISSUE = 0, C64_WRITE = 1, C64_READ = 2, C64_BARRIER = 3 };
constexpr int C64_EVENT_INTS = 6;

// Emits the events of `role` in program order through put(role, kind, halo, set, buf, tile); returns their number.
template <class Put>
inline int c64_emit_schedule(int role, int nsteps, int depth, Put put) {
  int n = 0;
  auto ev = [&](int kind, int halo) {
    const bool mem = kind != C64_BARRIER;
    put(role, kind, mem ? halo : -1, mem && kind != C64_READ ? c64_reg_set(halo, depth) : -1,
        kind == C64_WRITE || kind == C64_READ ? c64_lds_buf(halo) : -1, mem ? c64_tile_of_halo(halo, nsteps) : -1);
    ++n;
  };
  if (role == C64_PRODUCER) {
    for (int h = 0; h < depth - 1; ++h) ev(C64_ISSUE, h);
    ev(C64_WRITE, 0);
    ev(C64_ISSUE, depth - 1);
    ev(C64_BARRIER, 0);
    const int padded = c64_padded_steps(nsteps, depth);
    for (int s = 0; s < padded; ++s) {
      ev(C64_ISSUE, c64_issued_in_step(s, depth));
      ev(C64_WRITE, c64_written_in_step(s));
      ev(C64_BARRIER, 0);
    }
    ev(C64_BARRIER, 0);
  } else {
    ev(C64_BARRIER, 0);
    for (int s = 0; s < nsteps; ++s) {
      ev(C64_READ, s);
      ev(C64_BARRIER, 0);
    }
    for (int p = 0; p < c64_consumer_pad_barriers(nsteps, depth); ++p) ev(C64_BARRIER, 0);
    ev(C64_BARRIER, 0);
  }
  return n;
}

}  // namespace prg
