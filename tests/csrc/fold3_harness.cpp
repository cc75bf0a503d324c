// fold3_harness.cpp -- GPU test harness of the walker's three-input packed
// maximum (pk_max3_f16 of lx_internal.h, the F3 fold of index_body): the
// kernels here call the same __forceinline__ helper on raw words.  Test
// infrastructure only (tests/test_gpu_fold3_primitive.py).
//   f3h_apply: out[i] = pk_max3_f16(a[i], b[i], c[i]) for host arrays (the
//     test compares with the integer maximum of both halves in numpy);
//   f3h_pairs: every pair (x, y) in [0, lim)^2 in both halves (words
//     x | y << 16 and y | x << 16) with a zero third operand in each of the
//     three operand positions, checked on the device against the integer
//     maximum: res = {checked, bad, first bad: position, x, y, got}.
#include <hip/hip_runtime.h>

#include <string>

#include "lx_internal.h"

namespace {

std::string g_err;

int fail(int rc, const std::string &m) {
    g_err = m;
    return rc;
}

#define F3_HIP(x)                                                                  \
    do {                                                                           \
        hipError_t e_ = (x);                                                       \
        if (e_ != hipSuccess) return fail(-2, std::string(#x ": ") + hipGetErrorString(e_)); \
    } while (0)

__global__ void k_f3_apply(const uint32_t *a, const uint32_t *b, const uint32_t *c, uint64_t n, uint32_t *out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = pk_max3_f16(a[i], b[i], c[i]);
}

// workgroup x, lanes over y
__global__ void k_f3_pairs(uint32_t lim, unsigned long long *res) {
    const uint32_t x = blockIdx.x;
    uint32_t checked = 0;
    for (uint32_t y = threadIdx.x; y < lim; y += blockDim.x) {
        const uint32_t wa = x | y << 16, wb = y | x << 16;
        const uint32_t m = x > y ? x : y, want = m | m << 16;
        const uint32_t got[3] = {pk_max3_f16(0u, wa, wb), pk_max3_f16(wa, 0u, wb), pk_max3_f16(wa, wb, 0u)};
        for (int p = 0; p < 3; p++) {
            checked++;
            if (got[p] == want) continue;
            if (atomicAdd(res + 1, 1ull) == 0ull) {
                res[2] = p; res[3] = x; res[4] = y; res[5] = got[p];
            }
        }
    }
    atomicAdd(res + 0, (unsigned long long)checked);
}

template <class T>
struct Dev {
    T *p = nullptr;
    ~Dev() {
        if (p) (void)hipFree(p);
    }
};

}  // namespace

extern "C" const char *f3h_last_error() { return g_err.c_str(); }

extern "C" int f3h_apply(const uint32_t *a, const uint32_t *b, const uint32_t *c, uint64_t n, uint32_t *out) {
    if (!a || !b || !c || !out || !n || n > (1ull << 28)) return fail(-1, "f3h_apply: bad arguments");
    Dev<uint32_t> d[4];
    for (auto &x : d) F3_HIP(hipMalloc(reinterpret_cast<void **>(&x.p), n * 4));
    const uint32_t *src[3] = {a, b, c};
    for (int k = 0; k < 3; k++) F3_HIP(hipMemcpy(d[k].p, src[k], n * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_f3_apply, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, 0, d[0].p, d[1].p, d[2].p, n, d[3].p);
    F3_HIP(hipGetLastError());
    F3_HIP(hipMemcpy(out, d[3].p, n * 4, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int f3h_pairs(uint32_t lim, uint64_t *res) {
    if (!res || !lim || lim > 0x10000u) return fail(-1, "f3h_pairs: bad arguments");
    Dev<unsigned long long> d;
    F3_HIP(hipMalloc(reinterpret_cast<void **>(&d.p), 6 * 8));
    F3_HIP(hipMemset(d.p, 0, 6 * 8));
    hipLaunchKernelGGL(k_f3_pairs, dim3(lim), dim3(256), 0, 0, lim, d.p);
    F3_HIP(hipGetLastError());
    F3_HIP(hipMemcpy(res, d.p, 6 * 8, hipMemcpyDeviceToHost));
    return 0;
}
