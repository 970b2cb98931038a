// Carve sub-arrays out of one staging block: a segment is named once, by the offset take() returns, and whatever reserves,
// copies into or points into the block uses that name (host and device blocks share the layout).  Plain C++, no HIP.
#pragma once

#include <cstddef>

namespace orbgpu {

struct Carver {
    size_t off = 0;  // the next segment's offset; after the last take(), the size of the block
    size_t align;    // of every segment, a power of two: 256 for the id tables' blocks, 16 for the solvers' (vector loads)
    explicit Carver(size_t alignment = 256) : align(alignment) {}
    size_t take(size_t bytes)
    {
        const size_t o = off;
        off = (off + bytes + align - 1) & ~(align - 1);
        return o;
    }
};

} // namespace orbgpu
