// Carve sub-arrays out of one staging block: a segment is named once, by the offset take() returns, and whatever reserves,
// copies into or points into the block uses that name (host and device blocks share the layout).  Plain C++, no HIP.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstring>

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

// The workspace of a batch of the graph optimisers (local_ba.hip, essential_graph.hip): what is uploaded, of every problem,
// then the kernel's scratch, of every problem; segments on multiples of 256 bytes, an empty one still one element long.
// Each buffer is named once, in a function that describes a problem's segments and runs twice: on a WorkPlan() it only
// measures (nothing is read or written; every pointer handed out is null), which gives upload_bytes() and total() for the
// reservation; on WorkPlan(measured, dev, blob) it copies the sources into the host blob -- upload_bytes() long and
// zero-filled by the caller, one copy to `dev` for the whole batch -- and hands out the device pointers.
struct WorkPlan {
    WorkPlan() = default;
    WorkPlan(const WorkPlan &measured, char *dev_base, char *host_blob)
        : scratch_base(measured.upload_bytes()), dev(dev_base), blob(host_blob)
    {
    }
    size_t upload_bytes() const { return up.off; }
    size_t total() const { return up.off + scratch.off; }

    // uploaded: `count` elements copied from src
    template <typename T> T *seg(size_t count, const T *src)
    {
        T *host;
        T *d = seg_in_place(count, host);
        if (host && count)
            memcpy(host, src, count * sizeof(T));
        return d;
    }
    // uploaded, filled by the caller at `host` (its place in the blob; null while measuring)
    template <typename T> T *seg_in_place(size_t count, T *&host)
    {
        const size_t o = up.take(std::max<size_t>(count, 1) * sizeof(T));
        host = blob ? reinterpret_cast<T *>(blob + o) : nullptr;
        return at<T>(o);
    }
    // scratch
    template <typename T> T *seg(size_t count) { return at<T>(scratch_base + scratch.take(std::max<size_t>(count, 1) * sizeof(T))); }

  private:
    Carver up{256}, scratch{256};  // scratch counts from the end of the batch's uploads, a multiple of 256 itself
    size_t scratch_base = 0;
    char *dev = nullptr, *blob = nullptr;
    template <typename T> T *at(size_t o) const { return dev ? reinterpret_cast<T *>(dev + o) : nullptr; }
};

} // namespace orbgpu
