// Probe (gfx950): v_mov_b32_dpp row_newbcast:n with row_mask:0xf bank_mask:0xf -- does lane n of every 16-lane DPP row
// reach all 16 lanes of that row?  Every lane holds its lane index, all 64 lanes enabled; expected destination in lane
// t: 16 (t / 16) + n.  n = 0, 4, 8, 12 are what the four-row min-sum body uses (minsum_diag_impl.hpp, bank_bcast); the
// same four through the compiler builtin, which is the form the kernel contains.
//   hipcc --offload-arch=gfx950 -O2 row_newbcast_probe.hip -o row_newbcast_probe
#include <hip/hip_runtime.h>
#include <cstdio>
__global__ void k(unsigned *o) {
  const unsigned v = threadIdx.x;
  unsigned r[8];
  // (inline asm: the compiler counts no wait states between the write of v and the DPP reads, hence the s_nop)
  asm volatile(
      "s_nop 1\n\t"
      "v_mov_b32_dpp %0, %4 row_newbcast:0 row_mask:0xf bank_mask:0xf\n\t"
      "v_mov_b32_dpp %1, %4 row_newbcast:4 row_mask:0xf bank_mask:0xf\n\t"
      "v_mov_b32_dpp %2, %4 row_newbcast:8 row_mask:0xf bank_mask:0xf\n\t"
      "v_mov_b32_dpp %3, %4 row_newbcast:12 row_mask:0xf bank_mask:0xf"
      : "=&v"(r[0]), "=&v"(r[1]), "=&v"(r[2]), "=&v"(r[3])
      : "v"(v));
  r[4] = static_cast<unsigned>(__builtin_amdgcn_mov_dpp(static_cast<int>(v), 0x150, 0xF, 0xF, true));
  r[5] = static_cast<unsigned>(__builtin_amdgcn_mov_dpp(static_cast<int>(v), 0x154, 0xF, 0xF, true));
  r[6] = static_cast<unsigned>(__builtin_amdgcn_mov_dpp(static_cast<int>(v), 0x158, 0xF, 0xF, true));
  r[7] = static_cast<unsigned>(__builtin_amdgcn_mov_dpp(static_cast<int>(v), 0x15C, 0xF, 0xF, true));
  for (int j = 0; j < 8; ++j) o[j * 64 + threadIdx.x] = r[j];
}
int main() {
  unsigned *o, h[8 * 64];
  if (hipMalloc(&o, sizeof(h)) != hipSuccess) { printf("no device memory\n"); return 2; }
  (void)hipMemset(o, 0xFF, sizeof(h));
  k<<<1, 64>>>(o);
  if (hipMemcpy(h, o, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess) { printf("copy failed\n"); return 2; }
  int bad_total = 0;
  for (int j = 0; j < 8; ++j) {
    const unsigned n = 4 * (j % 4);
    int bad = 0;
    for (unsigned t = 0; t < 64; ++t) bad += h[j * 64 + t] != 16 * (t / 16) + n;
    printf("%s row_newbcast:%-2u lanes 0 / 15 / 16 / 37 / 63 read %u / %u / %u / %u / %u; %d of 64 lanes differ from 16 (lane / 16) + %u\n",
           j < 4 ? "asm    " : "builtin", n, h[j * 64], h[j * 64 + 15], h[j * 64 + 16], h[j * 64 + 37], h[j * 64 + 63], bad, n);
    bad_total += bad;
  }
  printf(bad_total ? "FAIL\n" : "PASS: every lane of a DPP row reads lane n of its own row\n");
  return bad_total ? 1 : 0;
}
