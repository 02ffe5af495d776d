// dd_gcn.h -- the gfx950 constructs of the convolution kernels that have no C++ meaning (LDS-DMA, s_waitcnt, the LDS base address, buffer
// descriptors), behind macros and small inline functions;
// tests/host_emul compiles the same kernel sources for the HOST with -DDD_HOST_EMULATION and maps the macros onto a model of the wave's VMEM
// queue (tests/host_emul/hip/hip_runtime.h): s_waitcnt vmcnt(N) retires all but the newest N entries in issue order, an LDS-DMA lands either
// at issue or only when a wait retires it -- the two extremes the hardware's timing lies between.
#pragma once

#ifdef DD_HOST_EMULATION

#define DD_DYN_SMEM(name) extern __attribute__((aligned(16))) char name[]          /* the harness defines dd::smem */
#define DD_PIN_VGPR(x) ((void)(x))
#define DD_LDS_BASE(smem) 0u
#define DD_LDS_DMA16(smem, gsrc, ldst) hostemu::lds_dma16((smem), (ldst), (gsrc))
#define DD_WAIT_VM(n) hostemu::wait_vm(n)
#define DD_WAIT_VM_LGKM0(n) hostemu::wait_vm(n)
#define DD_WAIT_LGKM0() ((void)0)
#define DD_SCHED_FENCE() ((void)0)
#define DD_VMEM_LOADS_ISSUED(n) hostemu::vmem_loads_issued(n)
#define DD_GLOBAL_STORE16_UNTRACKED(ptr, v) (*reinterpret_cast<float4*>(ptr) = (v))
typedef hostemu::tr16_v2u dd_u32x2_t;
#define DD_CVT_PKNORM_I16(a, b) hostemu::cvt_pknorm_i16((a), (b))
#define DD_LDS_READ_TR16(smem, byte_off) hostemu::lds_read_tr16((smem) + (byte_off))
// Buffer addressing (see the device half below): the same address, base + per-lane offset + scalar offset + immediate, and the range check
// of the descriptor made LOUD -- an access that ends beyond the descriptor's size aborts the emulated run (the hardware would drop it
// silently).  Loads and the LDS-DMA take their slot in the work-item's VMEM queue exactly like the global forms they replace.
struct dd_buf_t { char* base; unsigned long long bytes; };
static inline dd_buf_t dd_make_buf(const void* base, unsigned long long bytes) { return dd_buf_t{const_cast<char*>(reinterpret_cast<const char*>(base)), bytes}; }
static inline char* dd_buf_addr(const dd_buf_t& d, unsigned voff, unsigned soff, unsigned imm, unsigned size, const char* what) {
  const unsigned long long off = (unsigned long long)voff + soff + imm;
  if (off + size > d.bytes) {
    fprintf(stderr, "hostemu: %s of %u bytes at offset %llu (lane %u + scalar %u + immediate %u) leaves its %llu-byte buffer\n", what, size, off, voff, soff, imm, d.bytes);
    abort();
  }
  return d.base + off;
}
static inline uint4 dd_buf_load16(const dd_buf_t& d, unsigned voff, unsigned soff, unsigned imm) { return *reinterpret_cast<const uint4*>(dd_buf_addr(d, voff, soff, imm, 16, "buffer load")); }
static inline uint2 dd_buf_load8(const dd_buf_t& d, unsigned voff, unsigned soff, unsigned imm) { return *reinterpret_cast<const uint2*>(dd_buf_addr(d, voff, soff, imm, 8, "buffer load")); }
static inline uint32_t dd_buf_load4(const dd_buf_t& d, unsigned voff, unsigned soff, unsigned imm) { return *reinterpret_cast<const uint32_t*>(dd_buf_addr(d, voff, soff, imm, 4, "buffer load")); }
static inline void dd_buf_store16(const dd_buf_t& d, unsigned voff, unsigned soff, unsigned imm, uint4 v) { *reinterpret_cast<uint4*>(dd_buf_addr(d, voff, soff, imm, 16, "buffer store")) = v; }
// NP consecutive 1-KiB pieces: piece c from buffer offset soff + 1024 c to LDS byte ldst + 1024 c (lane l: 16 bytes at + 16 l of both)
template <int NP> static inline void dd_buf_lds_dma16(char* smem, const dd_buf_t& d, unsigned lane16, unsigned soff, unsigned ldst) {
  for (int c = 0; c < NP; ++c) hostemu::lds_dma16(smem, ldst + 1024u * c, dd_buf_addr(d, lane16, soff, 1024u * c, 16, "LDS-DMA piece"));
}
typedef dd_buf_t dd_bufw_t;
#define dd_make_bufw dd_make_buf

#else

// the workgroup's dynamic LDS (size given at launch)
#define DD_DYN_SMEM(name) extern __shared__ __attribute__((aligned(16))) char name[]
// "this value lives in a VGPR from here on": an empty asm the optimiser cannot look through (keeps loads above the selects that consume them)
#define DD_PIN_VGPR(x) asm volatile("" : "+v"(x))
#define DD_LDS_BASE(smem) ((unsigned)(size_t)(__attribute__((address_space(3))) char*)(smem))
// one wave-instruction: lane l copies 16 bytes from its global address gsrc to LDS address ldst (wave-uniform, via M0) + 16 * l.
// Inline asm on purpose: with the __builtin form hipcc treats the DMA as an LDS write that may alias every later ds_read and drains
// vmcnt(0) right behind it.  hipcc does not count asm VMEM operations: every wait for a DMA is one of the explicit macros below.
#define DD_LDS_DMA16(smem, gsrc, ldst)                                                                                          \
  do {                                                                                                                          \
    unsigned keep_m0_;                                                                                                          \
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"       \
                 : "=&s"(keep_m0_) : "v"(gsrc), "s"(ldst) : "memory");                                                          \
  } while (0)
// Buffer addressing: a global access as (128-bit descriptor in SGPRs) + (32-bit per-lane byte offset) + (scalar byte offset) + (12-bit
// immediate) instead of a 64-bit per-lane address -- the per-lane part is computed once per tile, what changes from access to access is
// scalar or immediate, and the address arithmetic leaves the VALU.  One descriptor per (tensor, image): base and size in bytes (below
// 2^32: conv_plan_fits_buffer_addressing, dd_api_plans.cpp), both wave-uniform; an access at or beyond the size is dropped by the
// hardware (loads return 0).  The loads and stores are the compiler's builtins, so hipcc counts them in vmcnt like the global forms.
typedef __amdgpu_buffer_rsrc_t dd_buf_t;
typedef __attribute__((ext_vector_type(4))) unsigned dd_u32x4_t;
static __device__ __forceinline__ dd_buf_t dd_make_buf(const void* base, unsigned long long bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, (int)(unsigned)bytes, 0x00020000);
}
static __device__ __forceinline__ uint4 dd_buf_load16(dd_buf_t d, unsigned voff, unsigned soff, unsigned imm) {
  return __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(d, voff + imm, soff, 0));
}
static __device__ __forceinline__ uint2 dd_buf_load8(dd_buf_t d, unsigned voff, unsigned soff, unsigned imm) {
  return __builtin_bit_cast(uint2, __builtin_amdgcn_raw_buffer_load_b64(d, voff + imm, soff, 0));
}
static __device__ __forceinline__ uint32_t dd_buf_load4(dd_buf_t d, unsigned voff, unsigned soff, unsigned imm) {
  return __builtin_amdgcn_raw_buffer_load_b32(d, voff + imm, soff, 0);
}
static __device__ __forceinline__ void dd_buf_store16(dd_buf_t d, unsigned voff, unsigned soff, unsigned imm, uint4 v) {
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(dd_u32x4_t, v), d, voff + imm, soff, 0);
}
// The LDS-DMA through a descriptor (inline asm for the reason given at DD_LDS_DMA16; its descriptor is the four words themselves): NP <= 4
// consecutive 1-KiB pieces of one wave -- piece c copies buffer bytes [soff + 1024 c, + 1024) to LDS [ldst + 1024 c, + 1024), lane l its 16
// bytes at + lane16 = 16 l.  One M0 write for all of them: the instruction's immediate offset advances the buffer AND the LDS address.
typedef __attribute__((ext_vector_type(4))) int dd_bufw_t;
static __device__ __forceinline__ dd_bufw_t dd_make_bufw(const void* base, unsigned long long bytes) {
  const unsigned long long a = (unsigned long long)base;
  return dd_bufw_t{__builtin_amdgcn_readfirstlane((int)(unsigned)a), __builtin_amdgcn_readfirstlane((int)(unsigned)(a >> 32)),
                   __builtin_amdgcn_readfirstlane((int)(unsigned)bytes), 0x00020000};
}
#define DD_BUF_DMA_PIECE_(imm) "\n\tbuffer_load_dwordx4 %1, %2, %3 offen offset:" #imm " lds"
template <int NP> static __device__ __forceinline__ void dd_buf_lds_dma16(char* /*smem*/, dd_bufw_t d, unsigned lane16, unsigned soff, unsigned ldst) {
  static_assert(NP >= 1 && NP <= 4, "the immediate offset has 12 bits");
  unsigned keep_m0_;
  if constexpr (NP == 1)
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %4\n\ts_nop 0" DD_BUF_DMA_PIECE_(0) "\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep_m0_) : "v"(lane16), "s"(d), "s"(soff), "s"(ldst) : "memory");
  else if constexpr (NP == 2)
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %4\n\ts_nop 0" DD_BUF_DMA_PIECE_(0) DD_BUF_DMA_PIECE_(1024) "\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep_m0_) : "v"(lane16), "s"(d), "s"(soff), "s"(ldst) : "memory");
  else if constexpr (NP == 3)
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %4\n\ts_nop 0" DD_BUF_DMA_PIECE_(0) DD_BUF_DMA_PIECE_(1024) DD_BUF_DMA_PIECE_(2048) "\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep_m0_) : "v"(lane16), "s"(d), "s"(soff), "s"(ldst) : "memory");
  else
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %4\n\ts_nop 0" DD_BUF_DMA_PIECE_(0) DD_BUF_DMA_PIECE_(1024) DD_BUF_DMA_PIECE_(2048) DD_BUF_DMA_PIECE_(3072) "\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep_m0_) : "v"(lane16), "s"(d), "s"(soff), "s"(ldst) : "memory");
}
#define DD_WAIT_VM(n) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(n) : "memory")
#define DD_WAIT_VM_LGKM0(n) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(n) : "memory")
#define DD_WAIT_LGKM0() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")
// nothing is scheduled across this point: keeps a burst of independent loads in front of the first code that waits for one of them
#define DD_SCHED_FENCE() __builtin_amdgcn_sched_barrier(0)
// A 16-byte global store the compiler does NOT see (inline asm).  hipcc keeps ONE vmcnt for loads and stores; once a store is pending beside
// loads it can no longer count ("counter out of order") and waits vmcnt(0) for the next load it needs -- which drains every prefetched load
// of a software pipeline.  Hidden from it, the store only makes its counted waits for loads more conservative (the hardware counter is
// higher than it assumes); the data is in memory by the end of the kernel like any other store.  The trailing `s_nop 1` keeps the two wait
// states gfx940+ needs between a VMEM store of more than 64 bits and a VALU write to its data registers: the hazard recogniser does not
// look into asm, and the next loop trip may recompute the same VGPRs right behind the store.
typedef __attribute__((ext_vector_type(4))) float dd_f32x4_t;
#define DD_GLOBAL_STORE16_UNTRACKED(ptr, v)                                                                                     \
  do {                                                                                                                          \
    const float4 f4_ = (v);                                                                                                     \
    const dd_f32x4_t v_ = {f4_.x, f4_.y, f4_.z, f4_.w};                                                                         \
    asm volatile("global_store_dwordx4 %0, %1, off\n\ts_nop 1" ::"v"(ptr), "v"(v_) : "memory");                                   \
  } while (0)
// v_cvt_pknorm_i16_f32: two floats in [-1, 1] -> two signed normalised 16-bit integers round(x * 32767), packed (lo = a)
#define DD_CVT_PKNORM_I16(a, b) __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pknorm_i16((a), (b)))
// bookkeeping for the host model only: n ordinary global loads were just issued by this wave (they count in vmcnt)
#define DD_VMEM_LOADS_ISSUED(n) ((void)0)
// ds_read_b64_tr_b16: the lane's 8-byte-aligned LDS address -> 4 x 16 bit, transposed inside each group of 16 lanes (see dd_wgrad2.hip)
typedef __attribute__((ext_vector_type(4))) short dd_s16x4_t;
typedef __attribute__((ext_vector_type(2))) unsigned dd_u32x2_t;
#define DD_LDS_READ_TR16(smem, byte_off)                                                                                              \
  __builtin_bit_cast(dd_u32x2_t, __builtin_amdgcn_ds_read_tr16_b64_v4i16(                                                             \
      (__attribute__((address_space(3))) dd_s16x4_t*)((__attribute__((address_space(3))) char*)(smem) + (byte_off))))

#endif
