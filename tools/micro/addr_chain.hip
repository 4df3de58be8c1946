// What one step of serial integer address generation costs on gfx950: one wavefront, a dependent chain of N steps, in four variants
//   plain    x = ((x + s) ^ 1) & 0xffff                        s a uniform in a scalar register
//   reload   the same, s read back from a lane of a vector register first (v_readlane_b32 + the wait states before its use):
//            what a scalar spilled to a lane costs where it is used
//   mul32    x = (x * s + 1) & 0xffff with the full 32-bit multiply (v_mul_lo_u32)
//   mul24    the same with the 24-bit multiply (v_mul_u32_u24)
// Prints ticks of the cycle counter per step; the differences reload - plain and mul32 - mul24 are what DESIGN.md section 4 ("scalar
// budget of the Newton loop") prices.
// Build: hipcc --offload-arch=gfx950 -O3 tools/micro/addr_chain.hip -o tools/micro/addr_chain
#include <hip/hip_runtime.h>
#include <cstdio>

template <int KIND> __global__ void chain(unsigned *out, long long *cyc, int iters, unsigned s_in)
{
    unsigned x = threadIdx.x, s = s_in;
    unsigned lanes = s_in + (threadIdx.x == 5 ? 0u : 7u);      // lane 5 holds s
    asm volatile("" : "+s"(s));
    long long t0 = __builtin_readcyclecounter();
    for (int i = 0; i < iters; ++i) {
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            if (KIND == 0) x = ((x + s) ^ 1u) & 0xffffu;
            if (KIND == 1) {
                asm volatile("" : "+v"(lanes));      // (not hoisted: a fresh reload per step, as in a loop under register pressure)
                const unsigned r = (unsigned)__builtin_amdgcn_readlane((int)lanes, 5);
                x = ((x + r) ^ 1u) & 0xffffu;
            }
            if (KIND == 2) x = (x * s + 1u) & 0xffffu;
            if (KIND == 3) x = (__umul24(x, s) + 1u) & 0xffffu;
        }
    }
    long long t1 = __builtin_readcyclecounter();
    out[threadIdx.x] = x;
    if (threadIdx.x == 0) cyc[0] = t1 - t0;
}

#define CK(e) do { hipError_t r_ = (e); if (r_ != hipSuccess) { printf("HIP error %s at line %d\n", hipGetErrorString(r_), __LINE__); return 1; } } while (0)

int main()
{
    unsigned *out; long long *cyc, h = 0;
    CK(hipMalloc(&out, 64 * sizeof(unsigned)));
    CK(hipMalloc(&cyc, sizeof(long long)));
    const int iters = 20000;        // x 16 unrolled steps
    const char *names[4] = {"plain", "reload", "mul32", "mul24"};
    unsigned ref[4] = {0, 0, 0, 0};
    for (int rep = 0; rep < 2; ++rep)       // the first round loads the code
        for (int k = 0; k < 4; ++k) {
            if (k == 0) hipLaunchKernelGGL(chain<0>, dim3(1), dim3(64), 0, 0, out, cyc, iters, 3u);
            if (k == 1) hipLaunchKernelGGL(chain<1>, dim3(1), dim3(64), 0, 0, out, cyc, iters, 3u);
            if (k == 2) hipLaunchKernelGGL(chain<2>, dim3(1), dim3(64), 0, 0, out, cyc, iters, 3u);
            if (k == 3) hipLaunchKernelGGL(chain<3>, dim3(1), dim3(64), 0, 0, out, cyc, iters, 3u);
            CK(hipDeviceSynchronize());
            CK(hipMemcpy(&h, cyc, sizeof h, hipMemcpyDeviceToHost));
            CK(hipMemcpy(&ref[k], out + 9, sizeof(unsigned), hipMemcpyDeviceToHost));
            if (rep) printf("%-7s %8.3f ticks per step\n", names[k], (double)h / (16.0 * iters));
        }
    if (ref[0] != ref[1] || ref[2] != ref[3]) { printf("variants disagree: %u %u %u %u\n", ref[0], ref[1], ref[2], ref[3]); return 1; }
    return 0;
}
