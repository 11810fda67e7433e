// mbd_debug_math.hip — the arithmetic primitives of mbd_math.h evaluated over arrays, one thread per element
// (include/mbd_hip_debug.h: mbd_debug_eval_math).  A test entry: tests/test_gpu_math.py holds every primitive, scalar and
// packed, to the checker's copy of the contract (spec_math.h, orc_sp_eval: the same op names) bit for bit and to
// float64 bounds.  Built with the library's flags and through its assembly pass, so it tests the code as shipped.
#include "mbd_internal.h"

namespace {

// name, inputs and outputs per element.  Packed ops ("...2", "div2x2_...") take elements (2j, 2j+1) as the low and high
// halves of their f2 operands, so their outputs line up with the scalar op's on the same array.
struct MathOp {
  const char* name;
  int k_in, k_out;
};
constexpr MathOp kMathOps[] = {
    {"rcp_exact", 1, 1},       {"div_", 2, 1},          {"div_pos_", 2, 1},       {"div2_", 2, 1},
    {"div2_pos_", 2, 1},       {"div2_sp_", 2, 1},      {"div2x2_", 4, 2},        {"div2x2_sp_", 4, 2},
    {"sqrt_floor", 1, 1},      {"angle_unit", 2, 1},    {"angle_unit_cpos", 2, 1}, {"angle_unit2", 2, 1},
    {"sincos_", 1, 2},         {"exp_", 1, 1},          {"log_", 1, 1},           {"log1p_", 1, 1},
    {"erfinv_", 1, 1},         {"bits_to_uniform", 3, 1}, {"bits_to_normal", 1, 1}, {"qnormalize", 4, 4},
    {"qnormalize_qm<1>", 4, 5}, {"qnormalize_qm<2>", 4, 4}, {"qrotvec_raw", 7, 4},   {"qrotvec", 7, 4},
    {"rot", 7, 3},             {"irot", 7, 3},          {"irot_z", 5, 3},         {"qmul", 8, 4},
    {"qaxes", 4, 9},           {"dot", 6, 1},           {"cross", 6, 3},          {"rot2", 7, 3},
    {"qmul2", 8, 4},           {"qaxes2", 4, 9},        {"dot2", 6, 1},           {"cross2", 6, 3},
    {"fmin_", 2, 1},           {"fmax_", 2, 1},         {"fclip", 3, 1},
};
constexpr int kNumMathOps = (int)(sizeof(kMathOps) / sizeof(kMathOps[0]));

int find_math_op(const char* name) {
  for (int k = 0; k < kNumMathOps; ++k)
    if (std::strcmp(kMathOps[k].name, name) == 0) return k;
  return -1;
}

__device__ __forceinline__ v3 ld3(const float* a) { return v3{a[0], a[1], a[2]}; }
__device__ __forceinline__ q4 ld4(const float* a) { return q4{a[0], a[1], a[2], a[3]}; }
__device__ __forceinline__ void st3(float* o, v3 v) { o[0] = v.x; o[1] = v.y; o[2] = v.z; }
__device__ __forceinline__ void st4(float* o, q4 q) { o[0] = q.w; o[1] = q.x; o[2] = q.y; o[3] = q.z; }

__global__ void eval_math_kernel(int op, long long n, int k_in, int k_out, const float* __restrict__ in,
                                 float* __restrict__ out) {
  const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  // the packed ops: this element is the low half (even j) or the high half of a pair; a lone last element pairs with itself
  const long long p = (j ^ 1) < n ? (j ^ 1) : j;
  const bool lo = (j & 1) == 0;
  const float* a = in + j * k_in;
  const float* b = in + p * k_in;
  float* o = out + j * k_out;
  auto pk = [&](int c) { return lo ? mk2(a[c], b[c]) : mk2(b[c], a[c]); };
  auto half = [&](f2 v) { return lo ? v.x : v.y; };
  auto pk3 = [&](int c) { return v3x2{pk(c), pk(c + 1), pk(c + 2)}; };
  auto pk4 = [&](int c) { return q4x2{pk(c), pk(c + 1), pk(c + 2), pk(c + 3)}; };
  auto st3x2 = [&](float* d, v3x2 v) { d[0] = half(v.x); d[1] = half(v.y); d[2] = half(v.z); };
  switch (op) {  // (case = index in kMathOps)
    case 0: o[0] = rcp_exact(a[0]); break;
    case 1: o[0] = div_(a[0], a[1]); break;
    case 2: o[0] = div_pos_(a[0], a[1]); break;
    case 3: o[0] = half(div2_(pk(0), pk(1))); break;
    case 4: o[0] = half(div2_pos_(pk(0), pk(1))); break;
    case 5: o[0] = half(div2_sp_(pk(0), pk(1))); break;
    case 6:
    case 7: {
      f2 qa, qb;
      if (op == 6) div2x2_(pk(0), pk(1), pk(2), pk(3), qa, qb);
      else div2x2_sp_(pk(0), pk(1), pk(2), pk(3), qa, qb);
      o[0] = half(qa);
      o[1] = half(qb);
      break;
    }
    case 8: o[0] = sqrt_floor(a[0]); break;
    case 9: o[0] = angle_unit(a[0], a[1]); break;
    case 10: o[0] = angle_unit_cpos(a[0], a[1]); break;
    case 11: o[0] = half(angle_unit2(pk(0), pk(1))); break;
    case 12: sincos_(a[0], &o[0], &o[1]); break;
    case 13: o[0] = exp_(a[0]); break;
    case 14: o[0] = log_(a[0]); break;
    case 15: o[0] = log1p_(a[0]); break;
    case 16: o[0] = erfinv_(a[0]); break;
    case 17: o[0] = bits_to_uniform(__builtin_bit_cast(uint32_t, a[0]), a[1], a[2]); break;
    case 18: o[0] = bits_to_normal(__builtin_bit_cast(uint32_t, a[0])); break;
    case 19: st4(o, qnormalize(ld4(a))); break;
    case 20: {
      float worst = 0.0f;
      st4(o, qnormalize_qm<1>(ld4(a), worst));
      o[4] = worst;
      break;
    }
    case 21: {
      float worst = 0.0f;
      st4(o, qnormalize_qm<2>(ld4(a), worst));
      break;
    }
    case 22: st4(o, qrotvec_raw(ld4(a), ld3(a + 4))); break;
    case 23: st4(o, qrotvec(ld4(a), ld3(a + 4))); break;
    case 24: st3(o, rot(ld3(a), ld4(a + 3))); break;
    case 25: st3(o, irot(ld3(a), ld4(a + 3))); break;
    case 26: st3(o, irot_z(a[0], ld4(a + 1))); break;
    case 27: st4(o, qmul(ld4(a), ld4(a + 4))); break;
    case 28: {
      const axes3 x = qaxes(ld4(a));
      st3(o, x.X); st3(o + 3, x.Y); st3(o + 6, x.Z);
      break;
    }
    case 29: o[0] = dot(ld3(a), ld3(a + 3)); break;
    case 30: st3(o, cross(ld3(a), ld3(a + 3))); break;
    case 31: st3x2(o, rot2(pk3(0), pk4(3))); break;
    case 32: {
      const q4x2 q = qmul2(pk4(0), pk4(4));
      o[0] = half(q.w); o[1] = half(q.x); o[2] = half(q.y); o[3] = half(q.z);
      break;
    }
    case 33: {
      const axes3x2 x = qaxes2(pk4(0));
      st3x2(o, x.X); st3x2(o + 3, x.Y); st3x2(o + 6, x.Z);
      break;
    }
    case 34: o[0] = half(dot2(pk3(0), pk3(3))); break;
    case 35: st3x2(o, cross2(pk3(0), pk3(3))); break;
    case 36: o[0] = fmin_(a[0], a[1]); break;
    case 37: o[0] = fmax_(a[0], a[1]); break;
    case 38: o[0] = fclip(a[0], a[1], a[2]); break;
    default: break;
  }
}

}  // namespace

extern "C" const char* mbd_debug_math_name(int k) { return k >= 0 && k < kNumMathOps ? kMathOps[k].name : nullptr; }

extern "C" int mbd_debug_math_arity(const char* op, int* k_in, int* k_out) {
  if (!op || !k_in || !k_out) return fail(MBD_ERR_INVALID, "NULL argument");
  const int id = find_math_op(op);
  if (id < 0) return fail(MBD_ERR_INVALID, "no math op named %s", op);
  *k_in = kMathOps[id].k_in;
  *k_out = kMathOps[id].k_out;
  return MBD_OK;
}

extern "C" int mbd_debug_eval_math(const char* op, long long n, const float* in, float* out) {
  if (!op) return fail(MBD_ERR_INVALID, "op is NULL");
  const int id = find_math_op(op);
  if (id < 0) return fail(MBD_ERR_INVALID, "no math op named %s", op);
  if (n < 0 || n > (1LL << 26)) return fail(MBD_ERR_INVALID, "eval_math: n=%lld outside [0, 2^26]", n);
  if (!in || !out) return fail(MBD_ERR_INVALID, "eval_math: NULL array");
  if (device_count_quiet() < 1) return fail(MBD_ERR_NO_DEVICE, "no HIP device: this library has no CPU fallback");
  if (n == 0) return MBD_OK;
  const int k_in = kMathOps[id].k_in, k_out = kMathOps[id].k_out;
  DevBuf<float> d_in, d_out;
  hipError_t e = d_in.upload(in, (size_t)n * k_in);
  if (e == hipSuccess) e = d_out.alloc((size_t)n * k_out);
  if (e == hipSuccess) {
    const int block = 256;
    hipLaunchKernelGGL(eval_math_kernel, dim3((unsigned)((n + block - 1) / block)), dim3(block), 0, 0, id, n, k_in, k_out, d_in.get(),
                       d_out.get());
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = d_out.download(out, (size_t)n * k_out);  // (a copy on the null stream: behind the kernel)
  if (e != hipSuccess) return fail(MBD_ERR_HIP, "eval_math(%s): %s", op, hipGetErrorString(e));
  return MBD_OK;
}
