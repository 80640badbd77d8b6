// Probe: which LDS bytes ds_read_b64_tr_b8 (the 8-bit transposed LDS read of gfx950) delivers to which lane and byte.
// Every lane l supplies the address of its own 8-byte chunk l of a 512-byte LDS image; the image is filled once with the
// chunk number and once with the byte position inside the chunk, so the two results name, for every (lane, result byte),
// the (supplying lane, byte of its chunk) it came from -- exact integer data, no arithmetic.  The whole wave is active
// (the instruction requires EXEC all ones) and every address is 8-byte aligned.
// Build: hipcc --offload-arch=gfx950 ds_read_tr8.hip -o bin/ds_read_tr8
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdint.h>
typedef __attribute__((ext_vector_type(2))) int v2i;

__global__ __launch_bounds__(64) void k_tr8(uint8_t* out) {
  __shared__ __attribute__((aligned(16))) uint8_t img[2][512];
  const int l = threadIdx.x;
  for (int j = 0; j < 8; ++j) { img[0][l * 8 + j] = (uint8_t)l; img[1][l * 8 + j] = (uint8_t)j; }
  __syncthreads();
  for (int p = 0; p < 2; ++p) {
    v2i r = __builtin_amdgcn_ds_read_tr8_b64_v2i32((__attribute__((address_space(3))) v2i*)(&img[p][l * 8]));
    *reinterpret_cast<v2i*>(out + (p * 64 + l) * 8) = r;
  }
}

int main() {
  uint8_t* d; uint8_t h[2][64][8];
  if (hipMalloc(&d, sizeof(h)) != hipSuccess) { printf("hipMalloc failed\n"); return 2; }
  hipLaunchKernelGGL(k_tr8, dim3(1), dim3(64), 0, 0, d);
  if (hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess) { printf("kernel or copy failed\n"); return 2; }
  printf("lane: result bytes 0..7 as supplier_lane.byte\n");
  for (int l = 0; l < 64; ++l) {
    printf("%2d:", l);
    for (int j = 0; j < 8; ++j) printf(" %2d.%d", h[0][l][j], h[1][l][j]);
    printf("\n");
  }
  // hypothesis A (the 8-bit analogue of the 16-bit form): per group of 16 lanes a block of 8 rows x 16 byte columns; lane 2q+p of the
  // group supplies row q, columns 8p..8p+7; lane i receives column i, row q in its byte q
  // hypothesis B: lane 8p+q supplies row q, columns 8p..8p+7
  int badA = 0, badB = 0;
  for (int l = 0; l < 64; ++l) for (int j = 0; j < 8; ++j) {
    const int g = l & ~15, i = l & 15;
    if (h[0][l][j] != g + 2 * j + (i >> 3) || h[1][l][j] != (i & 7)) ++badA;
    if (h[0][l][j] != g + 8 * (i >> 3) + j || h[1][l][j] != (i & 7)) ++badB;
  }
  printf("hypothesis A (lane 2q+p supplies row q, columns 8p..8p+7): %s (%d mismatches)\n", badA ? "NO" : "HOLDS", badA);
  printf("hypothesis B (lane 8p+q supplies row q, columns 8p..8p+7): %s (%d mismatches)\n", badB ? "NO" : "HOLDS", badB);
  hipFree(d);
  return 0;
}
