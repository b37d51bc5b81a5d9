// A 768-wide fp32 row held by one wave: 12 channels per lane as NV = 3 float4 (element lane + 64 i of the row's float4s), and how such
// a row is loaded and stored -- plain, non-temporal, as a 16-bit operand row, as a split-precision or f16 | e4m3 operand image.  Storage
// only: what a kernel computes on the row (statistics, LayerNorm bodies) stays with the kernel, whose rounding its own tests pin.
// Included by norm_elem.hip, fpool_transformer.hip and conformer.hip.
#pragma once
#include "common.h"

#define DM 768
#define NV 3  // float4 per lane per row

struct Row { float4 v[NV]; };

__device__ __forceinline__ float& f4(float4& v, int c) { return reinterpret_cast<float*>(&v)[c]; }
__device__ __forceinline__ const float& f4(const float4& v, int c) { return reinterpret_cast<const float*>(&v)[c]; }

__device__ __forceinline__ void row_load(Row& r, const float* p, int lane) {
#pragma unroll
    for (int i = 0; i < NV; ++i) r.v[i] = reinterpret_cast<const float4*>(p)[lane + 64 * i];
}
__device__ __forceinline__ void row_store(const Row& r, float* p, int lane) {
#pragma unroll
    for (int i = 0; i < NV; ++i) reinterpret_cast<float4*>(p)[lane + 64 * i] = r.v[i];
}
__device__ __forceinline__ void row_zero(float* p, int lane) {
    const float4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < NV; ++i) reinterpret_cast<float4*>(p)[lane + 64 * i] = z;
}
__device__ __forceinline__ void row_store_bf16(const Row& r, bf16_t* p, int lane, int f16) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        uint2 pk;
        pk.x = f16 ? pack2<true>(r.v[i].x, r.v[i].y) : pack2bf(r.v[i].x, r.v[i].y);
        pk.y = f16 ? pack2<true>(r.v[i].z, r.v[i].w) : pack2bf(r.v[i].z, r.v[i].w);
        reinterpret_cast<uint2*>(p)[lane + 64 * i] = pk;
    }
}
// Streaming variants: the activation rows these kernels walk are read once and written once; non-temporal accesses keep them from
// displacing each other in L2 (LayerNorm forward, cold input: 59.7 -> 33.7 us at M = 38080, 2.9 -> 5.2 TB/s; tools/ablate/ln_lab.hip).
typedef float f32x4nt __attribute__((ext_vector_type(4)));
typedef unsigned u32x2nt __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void row_load_nt(Row& r, const float* p, int lane) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const f32x4nt v = __builtin_nontemporal_load(reinterpret_cast<const f32x4nt*>(p) + lane + 64 * i);
        r.v[i] = make_float4(v[0], v[1], v[2], v[3]);
    }
}
__device__ __forceinline__ void row_store_nt(const Row& r, float* p, int lane) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const f32x4nt v = {r.v[i].x, r.v[i].y, r.v[i].z, r.v[i].w};
        __builtin_nontemporal_store(v, reinterpret_cast<f32x4nt*>(p) + lane + 64 * i);
    }
}
__device__ __forceinline__ void row_store_bf16_nt(const Row& r, bf16_t* p, int lane, int f16) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        u32x2nt pk;
        pk[0] = f16 ? pack2<true>(r.v[i].x, r.v[i].y) : pack2bf(r.v[i].x, r.v[i].y);
        pk[1] = f16 ? pack2<true>(r.v[i].z, r.v[i].w) : pack2bf(r.v[i].z, r.v[i].w);
        __builtin_nontemporal_store(pk, reinterpret_cast<u32x2nt*>(p) + lane + 64 * i);
    }
}
// split-precision operand image of a row: [hi | lo | hi] f16 over 3 * DM columns (what sed_split3_f16 makes in a pass of its own)
__device__ __forceinline__ void row_store_split3_nt(const Row& r, bf16_t* p, int lane) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const float v[4] = {r.v[i].x, r.v[i].y, r.v[i].z, r.v[i].w};
        bf16_t h[4], l[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) { h[e] = f2h(v[e]); l[e] = f2h(v[e] - h2f(h[e])); }
        u32x2nt hi, lo;
        hi[0] = (unsigned)h[0] | ((unsigned)h[1] << 16); hi[1] = (unsigned)h[2] | ((unsigned)h[3] << 16);
        lo[0] = (unsigned)l[0] | ((unsigned)l[1] << 16); lo[1] = (unsigned)l[2] | ((unsigned)l[3] << 16);
        u32x2nt* q = reinterpret_cast<u32x2nt*>(p) + lane + 64 * i;
        __builtin_nontemporal_store(hi, q);
        __builtin_nontemporal_store(lo, q + DM / 4);
        __builtin_nontemporal_store(hi, q + 2 * (DM / 4));
    }
}
// rows [DM f16 | DM e4m3] (pitch 3 DM / 2 halfs): the A operand of the two-term GEMMs with the lo product on the fp8 path (gemm_args.h
// GemmArgs.k8); the e4m3 half is 2^-2 x the f16-ROUNDED value (what sed_fp8_tail makes from the f16 half in a pass of its own)
__device__ __forceinline__ void row_store_f16_e4m3_nt(const Row& r, bf16_t* p, int lane) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const float v[4] = {r.v[i].x, r.v[i].y, r.v[i].z, r.v[i].w};
        bf16_t h[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) h[e] = f2h(v[e]);
        u32x2nt hi;
        hi[0] = (unsigned)h[0] | ((unsigned)h[1] << 16); hi[1] = (unsigned)h[2] | ((unsigned)h[3] << 16);
        __builtin_nontemporal_store(hi, reinterpret_cast<u32x2nt*>(p) + lane + 64 * i);
        __builtin_nontemporal_store(e4m3x4_of_h4(hi[0], hi[1]), reinterpret_cast<unsigned*>(p + DM) + lane + 64 * i);
    }
}
