// Probe: what the E8M0 block-scale operand of v_mfma_scale_f32_16x16x128_f8f6f4 does to an e4m3 product, with exact integer data.
// Claim to check (csrc/wgrad_patch_fp8.hip, the several-images-per-split instantiation): with the same byte in all four bytes of the A
// operand's scale register, uniform over the lanes, and 0x7f on the B side, D = C + (A x B) * 2^(byte - 127) -- exactly, for every byte
// the kernel can pass (exponent fields 1 .. 254 of a normal power-of-two float) as long as the result is a normal float, and the
// accumulator input C is NOT scaled.  Also: only byte 0 of the register matters for opsel 0, or all of them? (the kernel replicates the
// byte, so either answer is fine; printed for the record.)
// Build: hipcc --offload-arch=gfx950 fp8_mfma_scale.hip -o bin/fp8_mfma_scale
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
typedef __attribute__((ext_vector_type(8))) int v8i;
typedef __attribute__((ext_vector_type(4))) float v4f;

// OCP e4m3 bytes of the small exact values used here: k / 2 for k = -4 .. 4
static uint8_t enc_half(int k) {
  static const uint8_t pos[5] = {0x00, 0x30, 0x38, 0x3c, 0x40};   // 0, 0.5, 1, 1.5, 2
  return k < 0 ? (uint8_t)(0x80 | pos[-k]) : pos[k];
}

__global__ void k_mfma(const v8i* a, const v8i* b, const v4f* c, v4f* d, int sa, int sb) {
  d[threadIdx.x] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a[threadIdx.x], b[threadIdx.x], c[threadIdx.x], 0, 0, 0, sa, 0, sb);
}

int main() {
  // A[16][128] in {-2 .. 2} halves, B[128][16] in {-2 .. 2} halves; operand layout: lane l holds row / col l % 16, k = 32 * (l / 16) + byte
  std::vector<int> A(16 * 128), B(128 * 16);
  for (int i = 0; i < 16; ++i) for (int k = 0; k < 128; ++k) A[i * 128 + k] = ((i * 7 + k * 3) % 9) - 4;
  for (int k = 0; k < 128; ++k) for (int j = 0; j < 16; ++j) B[k * 16 + j] = ((k * 5 + j * 11) % 9) - 4;
  std::vector<double> P(256, 0.0);
  for (int i = 0; i < 16; ++i) for (int j = 0; j < 16; ++j) { double s = 0; for (int k = 0; k < 128; ++k) s += 0.25 * A[i * 128 + k] * B[k * 16 + j]; P[i * 16 + j] = s; }
  std::vector<uint8_t> ha(64 * 32), hb(64 * 32);
  for (int l = 0; l < 64; ++l) for (int q = 0; q < 32; ++q) {
    const int r = l % 16, k = 32 * (l / 16) + q;
    ha[l * 32 + q] = enc_half(A[r * 128 + k]);
    hb[l * 32 + q] = enc_half(B[k * 16 + r]);
  }
  std::vector<float> hc(256);
  for (int i = 0; i < 256; ++i) hc[i] = (float)((i % 5) - 2);       // accumulator input: small integers, must come through unscaled
  v8i *da, *db; v4f *dc, *dd;
  if (hipMalloc(&da, 64 * 32) != hipSuccess || hipMalloc(&db, 64 * 32) != hipSuccess || hipMalloc(&dc, 1024) != hipSuccess || hipMalloc(&dd, 1024) != hipSuccess) return 2;
  hipMemcpy(da, ha.data(), 64 * 32, hipMemcpyHostToDevice); hipMemcpy(db, hb.data(), 64 * 32, hipMemcpyHostToDevice);
  hipMemcpy(dc, hc.data(), 1024, hipMemcpyHostToDevice);
  int bad_total = 0;
  auto run = [&](int sa, int sb, double factor, const char* what) {
    hipLaunchKernelGGL(k_mfma, dim3(1), dim3(64), 0, 0, da, db, dc, dd, sa, sb);
    float hd[256];
    if (hipMemcpy(hd, dd, sizeof(hd), hipMemcpyDeviceToHost) != hipSuccess) { printf("launch failed\n"); bad_total += 1000; return; }
    int bad = 0; double maxabs = 0;
    for (int l = 0; l < 64; ++l) for (int r = 0; r < 4; ++r) {     // C / D layout: col = lane & 15, row = (lane >> 4) * 4 + reg
      const int row = (l >> 4) * 4 + r, col = l & 15;
      const double want = (double)hc[l * 4 + r] + P[row * 16 + col] * factor;
      if ((double)hd[l * 4 + r] != (double)(float)want) ++bad;
      maxabs = fmax(maxabs, fabs(want));
    }
    printf("scale_a=0x%08x scale_b=0x%08x  %-44s mismatches %3d / 256 (max |want| %.6g)\n", (unsigned)sa, (unsigned)sb, what, bad, maxabs);
    bad_total += bad;
  };
  // the accumulator input has at most 3 significant bits and the products 9: C + P * 2^e is exact in fp32 for |e| <= 12
  for (int byte : {127, 126, 125, 120, 117, 115, 128, 130, 139}) {
    char what[64];
    snprintf(what, sizeof(what), "byte %3d in all four bytes: C + P * 2^%d", byte, byte - 127);
    run(byte * 0x01010101, 0x7f7f7f7f, ldexp(1.0, byte - 127), what);
  }
  // far exponents: with a zero accumulator the scaled product alone is exact wherever it is a normal float
  hipMemset(dc, 0, 1024);
  std::fill(hc.begin(), hc.end(), 0.f);
  for (int byte : {4, 20, 64, 100, 200, 230}) {
    char what[64];
    snprintf(what, sizeof(what), "byte %3d, zero accumulator: P * 2^%d", byte, byte - 127);
    run(byte * 0x01010101, 0x7f7f7f7f, ldexp(1.0, byte - 127), what);
  }
  const int before = bad_total;
  // for the record only (not counted): which byte of the register is read when they differ
  run(0x7f7f7f7d, 0x7f7f7f7f, 0.25, "byte0 = 125, others 127: P / 4 if byte 0 is read");
  run(0x7d7f7f7f, 0x7f7f7f7f, 1.0, "byte3 = 125, others 127: P if byte 0 is read");
  bad_total = before;
  printf(bad_total == 0 ? "RESULT: D = C + (A x B) * 2^(byte - 127) exactly, C unscaled, for every replicated byte tried\n"
                        : "RESULT: MISMATCH (%d values)\n", bad_total);
  return bad_total == 0 ? 0 : 1;
}
