// The device side of a compaction (compact_plan.h plans it, id_table_compact in id_table.h is its transaction), shared
// by the observation graph and the key-frame database:
//   k_compact_pool<ELT...>  one wave per kept row, wave-uniform grid-stride (k_covis_vote's shape): the row's range of every
//                           pool column moves from the old buffers to freshly allocated ones -- no in-place hazard.  A
//                           column of ELT bytes per entry moves in the widest unit both sides are aligned for: 32-byte
//                           descriptors as 16-byte vectors (both offsets are multiples of 32 bytes), 8-byte ids and values
//                           as 8 bytes, 4-byte word ids as 4, attribute bytes as 4-byte words where both offsets are
//                           multiples of 4 and as bytes otherwise.  A lane issues four loads before the four stores.
//                           Rows that move nothing (length 0, kept bad rows) cost the three plan reads and no pool access.
//   k_compact_rows<Row>     new row i = old row src[i] with `off` rewritten from the plan (k_table_compact's manner).
//   k_compact_gather<T>     the same for a plain per-row column.
// Pure bandwidth; all global writes are plain vector stores.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace orbgpu {

constexpr int COMPACT_BLOCK = 256;
constexpr int COMPACT_WAVES = COMPACT_BLOCK / 64;

template <int N> struct CompactPool {
    const uint8_t *src[N];  // nullptr: the table does not have the column (yet)
    uint8_t *dst[N];
};

// n units of T from s to d, spread over the wave
template <typename T> __device__ __forceinline__ void compact_wave_copy(const T *__restrict__ s, T *__restrict__ d, int n, int lane)
{
    int i = lane;
    for (; i + 192 < n; i += 256) {
        const T a = s[i], b = s[i + 64], c = s[i + 128], e = s[i + 192];
        d[i] = a;
        d[i + 64] = b;
        d[i + 128] = c;
        d[i + 192] = e;
    }
    for (; i < n; i += 64)
        d[i] = s[i];
}

template <int ELT>
__device__ __forceinline__ void compact_copy_col(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, int64_t so, int64_t dn,
                                                 int len, int lane)
{
    static_assert(ELT == 1 || ELT == 4 || ELT == 8 || ELT % 16 == 0, "bytes per pool entry");
    if (!src)  // (kernel argument: wave-uniform)
        return;
    const uint8_t *s = src + so * ELT;
    uint8_t *d = dst + dn * ELT;
    if (ELT % 16 == 0)
        compact_wave_copy(reinterpret_cast<const uint4 *>(s), reinterpret_cast<uint4 *>(d), len * (ELT / 16), lane);
    else if (ELT == 8)
        compact_wave_copy(reinterpret_cast<const uint2 *>(s), reinterpret_cast<uint2 *>(d), len, lane);
    else if (ELT == 4)
        compact_wave_copy(reinterpret_cast<const uint32_t *>(s), reinterpret_cast<uint32_t *>(d), len, lane);
    else if (((so | dn) & 3) == 0) {  // the buffers are aligned as hipMalloc leaves them; offsets are wave-uniform
        const int words = len >> 2;
        compact_wave_copy(reinterpret_cast<const uint32_t *>(s), reinterpret_cast<uint32_t *>(d), words, lane);
        const int t = 4 * words + lane;
        if (t < len)
            d[t] = s[t];
    } else
        compact_wave_copy(s, d, len, lane);
}

// Kept row i moves len[i] entries from old_off[i] to new_off[i].  A range that does not lie inside both pools is passed
// over (the host plans inside them; a mistake there must not become a stray write).
template <int... ELT>
__global__ __launch_bounds__(COMPACT_BLOCK) void k_compact_pool(int n, const int64_t *__restrict__ old_off, const int64_t *__restrict__ new_off,
                                                               const int32_t *__restrict__ len, int64_t old_used, int64_t new_cap,
                                                               CompactPool<(int)sizeof...(ELT)> p)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int row = blockIdx.x * COMPACT_WAVES + wave; row < n; row += gridDim.x * COMPACT_WAVES) {  // wave-uniform
        const int l = len[row];
        const int64_t so = old_off[row], dn = new_off[row];
        if (l <= 0 || so < 0 || dn < 0 || so + l > old_used || dn + l > new_cap)
            continue;
        int c = 0;
        ((compact_copy_col<ELT>(p.src[c], p.dst[c], so, dn, l, lane), c++), ...);
    }
}

template <typename Row>
__global__ __launch_bounds__(256) void k_compact_rows(int n, const int32_t *__restrict__ src, const int64_t *__restrict__ new_off, int n_old,
                                                     const Row *__restrict__ o, Row *__restrict__ d)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || src[i] < 0 || src[i] >= n_old)
        return;
    Row r = o[src[i]];
    r.off = (decltype(r.off))new_off[i];
    d[i] = r;
}

template <typename T>
__global__ __launch_bounds__(256) void k_compact_gather(int n, const int32_t *__restrict__ src, int n_old, const T *__restrict__ o,
                                                       T *__restrict__ d)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && src[i] >= 0 && src[i] < n_old)
        d[i] = o[src[i]];
}

inline int compact_pool_grid(int n) { return n < COMPACT_WAVES * 2048 ? (n + COMPACT_WAVES - 1) / COMPACT_WAVES : 2048; }

} // namespace orbgpu
