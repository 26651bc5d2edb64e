#include <hip/hip_runtime.h>
#include <cstdio>
template <int CTRL> __global__ void k(int* out) { int x = threadIdx.x; out[threadIdx.x] = __builtin_amdgcn_update_dpp(-1, x, CTRL, 0xf, 0xf, false); }
__global__ void ksw16(int* out) {
    int a = threadIdx.x, b = threadIdx.x + 100;
    auto r = __builtin_amdgcn_permlane16_swap(a, b, false, false);
    out[threadIdx.x] = r[0]; out[64 + threadIdx.x] = r[1];
}
__global__ void ksw32(int* out) {
    int a = threadIdx.x, b = threadIdx.x + 100;
    auto r = __builtin_amdgcn_permlane32_swap(a, b, false, false);
    out[threadIdx.x] = r[0]; out[64 + threadIdx.x] = r[1];
}
// the tile butterfly's exchange over marker bit 3 as eval_body.h does it (lane_pair8_u32; eval_body's EPI_X8): the odd rows swap
// their quads j <-> j ^ 1 under a row mask, then v_permlane16_swap puts the two rows side by side
__global__ void kpair8(int* out) {
    const int x = threadIdx.x;
    const int a = __builtin_amdgcn_update_dpp(x, x, 0x141, 0xa, 0xf, false);                  // odd rows: row_half_mirror
    const unsigned z = (unsigned)__builtin_amdgcn_update_dpp(a, a, 0x1B, 0xa, 0xf, false);    // odd rows: quad_perm [3,2,1,0]
    auto r = __builtin_amdgcn_permlane16_swap(z, z, false, false);
    out[threadIdx.x] = r[0]; out[64 + threadIdx.x] = r[1];
}
// eval_body.h's lane <-> (marker, slot) map, restated
static void lane_map(int lane, int& m, int& g) {
    const int q = (lane >> 2) & 7, nib = (0x76452310u >> (4 * q)) & 7;
    g = (nib & 1) + 2 * (lane >> 5);
    m = ((nib >> 1) << 2) + (lane & 3);
}
static int lane_of(int m, int g) {
    const int idx = ((g & 1) << 2) + (m >> 2), q = (0x74216530u >> (4 * idx)) & 7;
    return ((g >> 1) << 5) + (q << 2) + (m & 3);
}
template <int CTRL> void run(const char* name) {
    int* d; hipMalloc(&d, 64 * 4); k<CTRL><<<1, 64>>>(d); int h[64]; hipMemcpy(h, d, 256, hipMemcpyDeviceToHost);
    printf("%s:", name); for (int i = 0; i < 32; ++i) printf(" %d", h[i]); printf("\n"); hipFree(d);
}
int main() {
    run<0x124>("row_ror4"); run<0x12C>("row_ror12"); run<0x128>("row_ror8"); run<0x104>("row_shl4"); run<0x114>("row_shr4");
    run<0x140>("row_mirror"); run<0x141>("row_half_mirror");
    int* d; hipMalloc(&d, 128 * 4); int h[128];
    ksw16<<<1, 64>>>(d); hipMemcpy(h, d, 512, hipMemcpyDeviceToHost);
    printf("permlane16_swap r0:"); for (int i = 0; i < 64; ++i) printf(" %d", h[i]); printf("\n r1:"); for (int i = 0; i < 64; ++i) printf(" %d", h[64 + i]); printf("\n");
    ksw32<<<1, 64>>>(d); hipMemcpy(h, d, 512, hipMemcpyDeviceToHost);
    printf("permlane32_swap r0:"); for (int i = 0; i < 64; ++i) printf(" %d", h[i]); printf("\n r1:"); for (int i = 0; i < 64; ++i) printf(" %d", h[64 + i]); printf("\n");
    // pair8: every lane of an EVEN row must hold {its own value, the value of the lane whose marker differs in bit 3, same slot};
    // the odd rows the same two values as the even row's lane at their position
    kpair8<<<1, 64>>>(d); hipMemcpy(h, d, 512, hipMemcpyDeviceToHost);
    int bad = 0;
    for (int i = 0; i < 64; ++i) {
        const int e = i & ~16;
        int m, g; lane_map(e, m, g);
        if (h[i] != e || h[64 + i] != lane_of(m ^ 8, g)) { ++bad; printf("pair8 lane %d: {%d, %d}, expected {%d, %d}\n", i, h[i], h[64 + i], e, lane_of(m ^ 8, g)); }
    }
    printf("pair8 (odd rows' quads j <-> j ^ 1, permlane16_swap): %s\n", bad ? "MISMATCH" : "ok, 64 lanes");
    hipFree(d);
    return bad ? 1 : 0;
}
