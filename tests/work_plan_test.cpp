// carve.h's WorkPlan on the CPU (g++ -fsanitize=address,undefined): for lists of segments, the offsets, upload_bytes() and
// total() of the two passes against a plain Carver(256) sequence in which every uploaded take precedes every scratch take;
// the blob (each source at its offset, zeros in the alignment gaps); the host address of a segment filled in place; and a
// measuring pass that reads no source -- its sources are one-byte heap blocks, so a copy would be a sanitizer report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "carve.h"

using orbgpu::Carver;
using orbgpu::WorkPlan;

#define CHECK(c)                                                                \
    do {                                                                        \
        if (!(c)) {                                                             \
            std::printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c);   \
            std::exit(1);                                                       \
        }                                                                       \
    } while (0)

struct Wide {
    uint64_t a, b;
};
enum Kind { COPIED, IN_PLACE, SCRATCH };
struct Seg {
    size_t size, count;
    Kind kind;
};
typedef std::vector<std::vector<Seg>> Batch;  // per problem, its segments in the order they are named

struct Named {
    const char *dev = nullptr;
    char *host = nullptr;  // IN_PLACE only
};

template <typename T> static Named name_one(WorkPlan &plan, const Seg &s, const char *src)
{
    Named n;
    if (s.kind == COPIED) {
        n.dev = reinterpret_cast<const char *>(plan.seg(s.count, reinterpret_cast<const T *>(src)));
    } else if (s.kind == IN_PLACE) {
        T *host;
        n.dev = reinterpret_cast<const char *>(plan.seg_in_place<T>(s.count, host));
        n.host = reinterpret_cast<char *>(host);
    } else {
        n.dev = reinterpret_cast<const char *>(plan.seg<T>(s.count));
    }
    return n;
}

// the describing function: every segment of every problem, once
static std::vector<Named> describe(WorkPlan &plan, const Batch &batch, const std::vector<const char *> &src)
{
    std::vector<Named> out;
    size_t i = 0;
    for (const std::vector<Seg> &problem : batch)
        for (const Seg &s : problem) {
            const char *from = src[i++];
            out.push_back(s.size == 1 ? name_one<uint8_t>(plan, s, from) : s.size == 4 ? name_one<uint32_t>(plan, s, from)
                          : s.size == 8 ? name_one<uint64_t>(plan, s, from) : name_one<Wide>(plan, s, from));
        }
    return out;
}

static char pattern(size_t seg, size_t byte) { return (char)(1 + (seg * 31 + byte * 7) % 250); }  // never 0

static void run(const Batch &batch)
{
    // the reference: a plain Carver(256), every uploaded take before every scratch take
    std::vector<Seg> flat;
    for (const std::vector<Seg> &problem : batch)
        flat.insert(flat.end(), problem.begin(), problem.end());
    std::vector<size_t> want(flat.size());
    Carver c(256);
    for (size_t i = 0; i < flat.size(); i++)
        if (flat[i].kind != SCRATCH)
            want[i] = c.take(std::max<size_t>(flat[i].count, 1) * flat[i].size);
    const size_t upload_bytes = c.off;
    for (size_t i = 0; i < flat.size(); i++)
        if (flat[i].kind == SCRATCH)
            want[i] = c.take(std::max<size_t>(flat[i].count, 1) * flat[i].size);
    const size_t total = c.off;

    // the measuring pass: null bases, sources that must not be read
    std::vector<std::unique_ptr<char[]>> tiny;
    std::vector<const char *> unreadable;
    for (size_t i = 0; i < flat.size(); i++) {
        tiny.emplace_back(new char[1]);
        unreadable.push_back(tiny.back().get());
    }
    WorkPlan measured;
    for (const Named &n : describe(measured, batch, unreadable))
        CHECK(n.dev == nullptr && n.host == nullptr);
    CHECK(measured.upload_bytes() == upload_bytes && measured.total() == total);

    // the second pass: the device block is never touched, so any address range of `total` bytes stands for it
    std::vector<std::vector<char>> source(flat.size());
    std::vector<const char *> src;
    for (size_t i = 0; i < flat.size(); i++) {
        source[i].resize(flat[i].count * flat[i].size);
        for (size_t b = 0; b < source[i].size(); b++)
            source[i][b] = pattern(i, b);
        src.push_back(source[i].data());
    }
    std::vector<char> dev(total), blob(upload_bytes, 0), expected(upload_bytes, 0);
    WorkPlan plan(measured, dev.data(), blob.data());
    const std::vector<Named> got = describe(plan, batch, src);
    CHECK(plan.upload_bytes() == upload_bytes && plan.total() == total);
    for (size_t i = 0; i < flat.size(); i++) {
        const size_t bytes = flat[i].count * flat[i].size;
        CHECK((size_t)(got[i].dev - dev.data()) == want[i] && want[i] % 256 == 0);
        CHECK(flat[i].kind == SCRATCH ? want[i] >= upload_bytes : want[i] + bytes <= upload_bytes);
        CHECK((got[i].host != nullptr) == (flat[i].kind == IN_PLACE));
        if (flat[i].kind == IN_PLACE) {
            CHECK(got[i].host == blob.data() + want[i]);
            if (bytes)
                memcpy(got[i].host, source[i].data(), bytes);  // the caller's conversion loop
        }
        if (flat[i].kind != SCRATCH && bytes)
            memcpy(expected.data() + want[i], source[i].data(), bytes);
    }
    CHECK(blob == expected);  // each source at its offset, zeros between
}

int main()
{
    const Batch empty = {{{4, 0, COPIED}, {8, 0, IN_PLACE}, {1, 0, SCRATCH}, {16, 0, COPIED}, {8, 0, SCRATCH}}};
    const Batch exact = {{{1, 256, COPIED}, {4, 64, COPIED}, {8, 32, IN_PLACE}, {16, 16, COPIED}, {8, 64, SCRATCH}, {1, 512, SCRATCH}}};
    const Batch one = {{{16, 3, COPIED}, {8, 33, SCRATCH}, {4, 65, COPIED}, {1, 7, SCRATCH}, {8, 5, IN_PLACE}, {1, 257, COPIED}}};
    const Batch three = {{{16, 3, COPIED}, {4, 65, COPIED}, {8, 5, IN_PLACE}, {8, 33, SCRATCH}, {1, 7, SCRATCH}},
                         {{16, 0, COPIED}, {4, 1, COPIED}, {8, 32, IN_PLACE}, {8, 0, SCRATCH}, {1, 256, SCRATCH}},
                         {{16, 17, COPIED}, {4, 63, COPIED}, {8, 31, IN_PLACE}, {8, 1, SCRATCH}, {1, 255, SCRATCH}}};
    for (const Batch &b : {empty, exact, one, three})
        run(b);
    run(Batch{});  // no problem at all: nothing uploaded, nothing reserved
    std::printf("work_plan_test ok\n");
    return 0;
}
