// Host-side helpers of the files that lower a model to launch sequences (encoder.hip, extractors.hip): zero-filled
// descriptors, the Linear builder and the workspace arena.  Host code only.
#pragma once
#include <string.h>

#include "common.h"

inline tribe_gemm_desc gemm_zero() {
  tribe_gemm_desc d;
  memset(&d, 0, sizeof(d));
  d.batch1 = d.batch0 = 1;
  d.alpha = 1.0f;
  d.c_dtype = TRIBE_F32;
  return d;
}

inline tribe_attention_desc attn_zero() {
  tribe_attention_desc a;
  memset(&a, 0, sizeof(a));
  return a;
}

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// One nn.Linear as a GEMM descriptor: C[M, N] = act(alpha * A[M, K] . W[N, K]^T + bias) (+ res), rows of A and W K wide, rows of C
// N wide.  What only some sites use (res_scale, row_scale, c_bf16 / row_sumsq, batches and strides, stream_k) is assigned on the result.
struct Linear : tribe_gemm_desc {
  Linear(int32_t role_, int64_t M_, const void* A_, int64_t K_, const void* W, const float* bias_, void* C_, int64_t N_, int32_t dtype)
      : tribe_gemm_desc(gemm_zero()) {
    M = M_; N = N_; K = K_;
    A = A_; lda = K_; B = W; ldb = K_;
    C = C_; ldc = N_; c_dtype = dtype;
    if (bias_) { bias = bias_; bias_mode = TRIBE_BIAS_COL; }
    role = role_;
  }
  // the gated activations (SwiGLU, GLU) store N / 2 columns: pass the stored width
  Linear& activation(int32_t a, int64_t stored_width = 0) {
    act = a;
    if (stored_width) ldc = stored_width;
    return *this;
  }
  Linear& residual(const float* r) { res = r; ldres = ldc; return *this; }   // after activation(): as wide as the stored rows
  Linear& scaled(float a) { alpha = a; return *this; }
};

// Workspace layout, written once per model as a function `layout(desc, Arena&)` that take()s its buffers in order: over nullptr
// it only measures (`off` is the workspace size, nothing is dereferenced), over the caller's workspace it hands out the pointers.
struct Arena {
  uintptr_t base;
  size_t off = 0;
  explicit Arena(void* workspace = nullptr) : base((uintptr_t)workspace) {}
  template <class T>
  T* take(size_t bytes) {
    T* p = (T*)(base + off);
    off += align256(bytes);
    return p;
  }
};
