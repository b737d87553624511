// A ring of LDS slots filled by global -> LDS loads with no register between:
// the pieces of the streaming CGS update (k_cgs_update_nc<..., STREAM>) and of
// the cycle's tail (k_update_tail_nc<..., STREAM>).
#pragma once

#include "internal.hpp"

namespace {

// Beside an LDS-DMA in flight the compiler waits vmcnt(0) at the first use of
// any load it counts and before every ds_read that may see a DMA's bytes, so
// the three accesses that must not drain the ring are kept out of its count:
// the partial loads, and the reads of a slot and of a coefficient. Each is
// paired with its own wait, stated where it is issued.
typedef __attribute__((address_space(3))) void* lds_ptr_t;
typedef float f32x4_t __attribute__((ext_vector_type(4)));
constexpr int kStreamSlots = 9;  // 16 KB each for 1024 lanes: 144 KB of the CU's 160 KB

// one partial, requested and not waited for (cgs_stream_wait_partials does).
// ASSUMPTION: the returned register is still being filled. The compiler takes
// it as written when the statement ends, and nothing but its one use -- the
// "+v" operand of cgs_stream_wait_partials -- orders a reader behind the
// load: the value must reach that statement in the register the load names,
// with no copy, spill or coalescing move between the two. The 8 values have
// no other use and are requested at the kernel's entry, far from any register
// pressure, and in the gfx950 code of every instance built the registers are
// untouched from the load to the wait; after a compiler change check that
// again (tools/kernel_resources.py for spills, the assembly between the
// global_load_dwordx2 group and the first s_waitcnt vmcnt for a v_mov).
__device__ __forceinline__ double cgs_stream_load_partial(const double* p) {
    double v;
    asm volatile("global_load_dwordx2 %0, %1, off" : "=v"(v) : "v"(p) : "memory");
    return v;
}
// the 8 partials have landed once at most BEHIND younger requests are pending
template <int BEHIND>
__device__ __forceinline__ void cgs_stream_wait_partials(double (&p)[8]) {
    asm volatile("s_waitcnt vmcnt(%8)"
                 : "+v"(p[0]), "+v"(p[1]), "+v"(p[2]), "+v"(p[3]), "+v"(p[4]), "+v"(p[5]), "+v"(p[6]), "+v"(p[7])
                 : "i"(BEHIND)
                 : "memory");
    __builtin_amdgcn_sched_barrier(0);
}
// the lane's 16 bytes of a slot and one coefficient, once at most BEHIND
// requests younger than the slot's own are pending; on return both reads have
// completed, so the slot may be requested again
template <int BEHIND>
__device__ __forceinline__ void cgs_stream_take(unsigned slot_lds, unsigned coef_lds, f32x4_t& v, float& cu) {
    asm volatile("s_waitcnt vmcnt(%4)\n\tds_read_b128 %0, %2\n\tds_read_b32 %1, %3\n\ts_waitcnt lgkmcnt(0)"
                 : "=&v"(v), "=&v"(cu)
                 : "v"(slot_lds), "v"(coef_lds), "i"(BEHIND)
                 : "memory");
    __builtin_amdgcn_sched_barrier(0);
}
// the lane's 16 bytes of a column, global -> LDS with no register between:
// one wave-instruction writes 1 KB at the wave-uniform `lds_wave` + lane * 16
__device__ __forceinline__ void cgs_stream_request(const float* g, unsigned lds_wave) {
    __builtin_amdgcn_global_load_lds(g, (lds_ptr_t)(size_t)lds_wave, 16, 0, 0);
}
// the sums so far are formed here (an empty statement the compiler cannot
// move the products across)
__device__ __forceinline__ void cgs_stream_pin(float (&t)[4]) {
    asm volatile("" : "+v"(t[0]), "+v"(t[1]), "+v"(t[2]), "+v"(t[3]));
}

}  // namespace
