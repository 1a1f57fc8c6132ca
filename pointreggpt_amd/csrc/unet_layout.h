// unet_layout.h — what the three HIP host units of the U-Nets share (unet.hip: forward pass, sampler, C-ABI; unet_weights.hip:
// upload of the weight arenas; unet_debug.hip: the prg_debug_* entries): owned device buffers and the prg_unet handle.  The
// parameter layout, its one traversal, the shape rules and every packer are host-only C++ and live in weights_host.h.
#pragma once
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "blocks.h"
#include "conv.h"
#include "weights_host.h"

namespace prg {

// build_layout (weights_host.h) behind prg_last_error, plus the one limit that belongs to the kernels and not to the layout
inline int build_layout_checked(const prg_unet_config& cfg, Layout& L) {
  std::string err;
  const int rc = build_layout(cfg, L, err);
  if (rc) return fail(rc, err);
  for (size_t i = 0; i < L.dims.size(); ++i)
    if (L.dims[i] > 1024)
      return fail(PRG_E_INVALID, "config: dim * dim_mult = " + std::to_string(L.dims[i]) + " exceeds 1024 channels, the widest "
                  "GroupNorm the coefficient kernels handle (gn_coeff_kernel / affine_silu_fold_kernel: four channels per thread)");
  return PRG_OK;
}

// ---------------------------------------------------------------------------------------------
// owned device allocations: freed when the owner goes (a handle, or the scope of a debug entry).  The first failure sticks in
// `rc` (and behind prg_last_error) and turns every later call into a no-op that returns null: check once after a group of calls.
// ---------------------------------------------------------------------------------------------
struct DeviceBuffers {
  std::vector<void*> ptrs;
  int rc = PRG_OK;
  DeviceBuffers() = default;
  DeviceBuffers(const DeviceBuffers&) = delete;
  DeviceBuffers& operator=(const DeviceBuffers&) = delete;
  ~DeviceBuffers() { for (void* p : ptrs) (void)hipFree(p); }
  // uninitialised device memory; `nomem` is the whole PRG_E_NOMEM message.  count == 0: null
  template <typename U>
  U* alloc(size_t count, const char* nomem) {
    void* p = nullptr;
    if (rc != PRG_OK || count == 0) return nullptr;
    if (hipMalloc(&p, count * sizeof(U)) != hipSuccess) { rc = fail(PRG_E_NOMEM, nomem); return nullptr; }
    ptrs.push_back(p);
    return static_cast<U*>(p);
  }
  // hipMalloc + hipMemcpy of `count` host elements
  template <typename U>
  U* upload(const U* src, size_t count, const char* nomem) {
    U* p = alloc<U>(count, nomem);
    if (p) {
      const hipError_t e = hipMemcpy(p, src, count * sizeof(U), hipMemcpyHostToDevice);
      if (e != hipSuccess) { rc = fail(PRG_E_HIP, std::string("hipMemcpy (") + nomem + "): " + hipGetErrorString(e)); return nullptr; }
    }
    return p;
  }
  template <typename U>
  U* upload(const std::vector<U>& v, const char* nomem) { return upload(v.data(), v.size(), nomem); }
};

// ---------------------------------------------------------------------------------------------
// device stack arena (the workspace of a handle)
// ---------------------------------------------------------------------------------------------
struct Arena {
  char* base = nullptr;
  size_t cap = 0, top = 0, high = 0;
  bool dry = false;  // dry run: only measure
  void* alloc(size_t bytes) {
    size_t a = (top + 255) & ~(size_t)255;
    top = a + bytes;
    if (top > high) high = top;
    if (dry) return reinterpret_cast<void*>((uintptr_t)0x1000 + a);  // never dereferenced
    return (top <= cap) ? base + a : nullptr;
  }
  size_t mark() const { return top; }
  void reset(size_t m) { top = m; }
};

// conditioning source for the ResnetBlocks of one forward
struct CondSrc {
  const float* ss_a = nullptr;
  const float* ss_b = nullptr;
  int64_t ss_a_stride = 0, ss_b_stride = 0;
  const int* row = nullptr;
  int64_t row_stride = 0;
};

struct Tap {
  const void* ptr;
  int C, H, W, B;
  bool nchw_f32;
};

struct ProfileSink;   // per-launch conv timing (unet.hip)

}  // namespace prg

// ---------------------------------------------------------------------------------------------
// the U-Net handle.  `own` holds every weight buffer; the typed d_* members below are views into it (null: the handle has no such
// packing).  The workspace and d_gnacc are reallocated by reserve() and freed by prg_unet_destroy.
// ---------------------------------------------------------------------------------------------
struct prg_unet {
  prg::Layout lay;
  int dtype = PRG_F32;
  prg::DeviceBuffers own;
  float* d_flat = nullptr;      // the float32 state_dict on device (biases, norm gains, MLPs read in place)
  void* d_packed = nullptr;     // packed conv weights of T
  float* d_stem = nullptr;      // stem weights [49*Cin][dim]
  prg::bf16_t* d_stem_frag = nullptr; // stem weights as MFMA fragments (bf16 path, Cin 1 -> 64)
  uint16_t* d_stem_split = nullptr;    // f16x3 mode: the same fragments as f16 hi / lo halves (stem_mfma_kernel<CIN, true>)
  float* d_stem_split_scale = nullptr; // ... and the inverse of the packer's per-channel power-of-two scale [64]
  prg::bf16_t* d_attn = nullptr;     // fused linear attention: gain-folded to_qkv and to_out weights (bf16 path only)
  float* d_kshift = nullptr;    // fused linear attention: static softmax shifts of the k columns
  uint8_t* d_mx = nullptr;      // MX-fp8 conv weights (dtype PRG_MXFP8): e4m3 data and E8M0 block scales
  uint8_t* d_mx_scale = nullptr;
  uint16_t* d_attn_split = nullptr;   // f16x3 mode: fused linear attention weights as f16 hi / lo halves (attn_split.hip)
  float* d_split_scale = nullptr;   // f16x3 mode: the packer's per-output-channel power-of-two factors, undone in the epilogues
  uint16_t* d_split = nullptr;  // f16x3 mode (dtype PRG_F16X3): every conv weight as f16 hi / lo halves (conv_split.hip)
  uint16_t* d_h16 = nullptr;    // bf16 mode: f16 twins of the ResnetBlocks' second convs (the h16 format, conv.h)
  float* d_freqs = nullptr;     // SinusoidalPosEmb frequencies [dim/2] (sd:645-657), see prg_unet_set_time_freqs
  // fixed-point GroupNorm statistics (common.h, GnFold; bf16 / mxfp8 handles)
  long long* d_gnacc = nullptr; // [slots][resB][groups][2], zeroed by ONE memset at the start of every forward
  size_t gnacc_bytes = 0;
  int gn_slots = 0, gn_slot = 0;
  float* d_pq_static = nullptr; // (gamma | beta) of every norm, 16-byte aligned rows: P / Q of the unconditioned norms
  prg::CondFoldEntry* d_cond_entries = nullptr;   // one entry per conditioned norm (Block 1 of every ResnetBlock)
  int n_cond_entries = 0;
  prg::Arena arena;
  uint64_t arena_gen = 0;       // bumped whenever the workspace is reallocated: captured graphs bake its pointers in
  int resB = 0, resS = 0;
  bool taps_on = false;
  std::map<std::string, prg::Tap> taps;
  prg::ProfileSink* prof = nullptr;
  virtual ~prg_unet() {}
  virtual int measure(int B, int S, size_t* bytes) = 0;
  virtual int forward(const float* x_nchw, const prg::CondSrc& cond, float* out, int B, int S, hipStream_t s) = 0;
  virtual int cond_general(const int64_t* time, const float* param_cond, int B, prg::CondSrc* out, hipStream_t s) = 0;
  virtual int tap_copy(const prg::Tap& t, float* out, hipStream_t s) = 0;
};

namespace prg {
// build_layout + every weight arena of a fresh handle (its storage type is given by dtype: float for PRG_F32 / PRG_F16X3,
// bf16_t for PRG_BF16 / PRG_MXFP8).  On failure the caller deletes the handle, which frees what was uploaded.
int prepare_unet_weights(prg_unet& u, const prg_unet_config& cfg, const float* weights, int64_t n, int dtype);
}  // namespace prg
