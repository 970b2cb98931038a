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

// The staging of a host flavour (sim3.hip, sim3_opt.hip, pnp.hip, initializer.hip, local_ba.hip, essential_graph.hip): every
// caller array is one segment of one of the workspace's buffers, declared once -- buffer, host pointer (may be null), rows,
// elements per row, direction -- and the declaration decides all that follows from it.  It reserves
// max(rows, 1) * max(width, 1) elements on a multiple of 16 bytes (an empty segment is still one element long: the kernels
// read with vector loads); it copies rows * width elements, and only when the host pointer is non-null and that is not
// zero.  The handle it returns carries buffer and offset: ws.at(handle) is the device pointer, and a row fetched after the
// launch takes its offset from the handle.  upload() / download() issue the copies in declaration order through whatever
// workspace they are given (Staging, or the recording one of tests/carve_test.cpp); N is the workspace's buffer count.
template <typename T> struct Seg {
    int buf;
    size_t off;
};

template <int N> struct HostPlan {
    static constexpr int MAX_SEGS = 16;  // the longest list (sim3.hip) has 13
    HostPlan()
    {
        for (Carver &c : carve)
            c.align = 16;
    }
    template <typename T> Seg<T> in(int buf, const T *host, size_t rows, size_t width = 1)
    {
        return add(buf, const_cast<T *>(host), rows, width, IN);
    }
    template <typename T> Seg<T> out(int buf, T *host, size_t rows, size_t width = 1) { return add(buf, host, rows, width, OUT); }
    template <typename T> Seg<T> inout(int buf, T *host, size_t rows, size_t width = 1) { return add(buf, host, rows, width, IN | OUT); }

    size_t bytes(int buf) const { return carve[buf].off; }  // of the buffer's block so far; 0: the plan does not use it
    bool ok() const { return !overflow; }  // false: a segment beyond MAX_SEGS was declared (carved, but never copied)
    template <typename Ws> void upload(Ws &ws) const
    {
        for (int i = 0; i < n; i++)
            if (rec[i].dir & IN)
                ws.upload(rec[i].buf, rec[i].host, rec[i].bytes, rec[i].off);
    }
    template <typename Ws> void download(Ws &ws) const
    {
        for (int i = 0; i < n; i++)
            if (rec[i].dir & OUT)
                ws.download(rec[i].host, rec[i].buf, rec[i].bytes, rec[i].off);
    }

  private:
    enum { IN = 1, OUT = 2 };
    struct Copy {
        void *host;
        size_t off, bytes;
        int buf, dir;
    };
    Carver carve[N];
    Copy rec[MAX_SEGS];
    int n = 0;
    bool overflow = false;
    template <typename T> Seg<T> add(int buf, T *host, size_t rows, size_t width, int dir)
    {
        const size_t off = carve[buf].take(std::max<size_t>(rows, 1) * std::max<size_t>(width, 1) * sizeof(T));
        const size_t bytes = rows * width * sizeof(T);
        if (host && bytes) {
            if (n < MAX_SEGS)
                rec[n++] = Copy{host, off, bytes, buf, dir};
            else
                overflow = true;
        }
        return Seg<T>{buf, off};
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
