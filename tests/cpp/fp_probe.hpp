// TEST INFRASTRUCTURE ONLY — shared by the two translation units of the field-layer probe (fp_probe.hip: the field ops and the
// C entry; fp_probe_group.hip: the group law and the limb-parallel code).  The probe includes the product's headers as they
// stand and hands every primitive raw limbs: no packing and no canonicalisation on the way in or out.
//
// Records are fixed-size arrays of uint32_t.  A field element is 9 limbs, an affine point 18 (x || y), an XYZZ point 36
// (x || y || zz || zzz), a flag one word.  One case per thread for the single-lane code, one case per wave for the
// limb-parallel code; the op is a template argument of the kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

namespace fp_probe {

struct Entry {
    const char* name;   // the op's name: what tests/fp_probe.py looks up
    int field;          // 0: Fq, 1: Fr
    int in_words, out_words;
    hipError_t (*run)(const uint32_t* host_in, uint32_t n, uint32_t* host_out);
};

// one case per thread
template <class Op>
__global__ void __launch_bounds__(64) k_probe(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t n) {
    const uint32_t t = blockIdx.x * 64u + threadIdx.x;
    if (t >= n) return;
    Op::run(in + (size_t)t * Op::IN, out + (size_t)t * Op::OUT);
}
// one case per wave (workgroup = one wave)
template <class Op>
__global__ void __launch_bounds__(64) k_probe_wave(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t n) {
    if (blockIdx.x >= n) return;
    Op::run(in + (size_t)blockIdx.x * Op::IN, out + (size_t)blockIdx.x * Op::OUT);
}

template <class Op, bool WAVE>
hipError_t launch(const uint32_t* host_in, uint32_t n, uint32_t* host_out) {
    if (n == 0) return hipSuccess;
    const size_t in_bytes = sizeof(uint32_t) * Op::IN * (size_t)n, out_bytes = sizeof(uint32_t) * Op::OUT * (size_t)n;
    uint32_t *din = nullptr, *dout = nullptr;
    hipError_t e = hipMalloc(&din, in_bytes);
    if (e == hipSuccess) e = hipMalloc(&dout, out_bytes);
    if (e == hipSuccess) e = hipMemcpy(din, host_in, in_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(dout, 0, out_bytes);
    if (e == hipSuccess) {
        if (WAVE) hipLaunchKernelGGL(k_probe_wave<Op>, dim3(n), dim3(64), 0, 0, din, dout, n);
        else hipLaunchKernelGGL(k_probe<Op>, dim3((n + 63u) / 64u), dim3(64), 0, 0, din, dout, n);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(host_out, dout, out_bytes, hipMemcpyDeviceToHost);
    if (din) (void)hipFree(din);
    if (dout) (void)hipFree(dout);
    return e;
}

inline const Entry* find(const Entry* table, int count, int field, const char* name) {
    for (int i = 0; i < count; ++i)
        if (table[i].field == field && strcmp(table[i].name, name) == 0) return &table[i];
    return nullptr;
}

// the second translation unit's table
const Entry* group_table(int* count);

}  // namespace fp_probe
