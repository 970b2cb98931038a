// carve.h on the CPU (g++ -fsanitize=address,undefined): the offsets Carver hands out at both alignments in use, and HostPlan
// driven through a recording workspace over the segment lists of the seven host flavours (orbgpu_sim3_solve*,
// orbgpu_sim3_optimize, orbgpu_pnp_solve*, orbgpu_initializer*, orbgpu_local_ba, orbgpu_bundle_adjustment,
// orbgpu_essential_graph), as tables read off the entry points as they were when each held its own take() / upload() /
// download() lines: offsets and block sizes against those hand-summed formulas, the copies against those guards.  The
// "device" blocks are heap blocks of exactly the reserved size and every caller array one of exactly its documented length,
// so a copy that is too long is an AddressSanitizer report.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "carve.h"
#include "orbgpu.h"

using orbgpu::Carver;
using orbgpu::HostPlan;

#define CHECK(c)                                                                \
    do {                                                                        \
        if (!(c)) {                                                             \
            std::printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c);   \
            std::exit(1);                                                       \
        }                                                                       \
    } while (0)

static void sequence(Carver c, size_t A)
{
    const size_t sizes[] = {0, 1, 15, 16, 17, 255, 256, 257};
    size_t prev = 0, end_of_last = 0;
    CHECK(c.off == 0);
    for (size_t bytes : sizes) {
        const size_t o = c.take(bytes);
        CHECK(o == prev && o % A == 0);
        CHECK(o >= end_of_last);  // no overlap with the segment before
        CHECK(c.off == ((prev + bytes + A - 1) & ~(A - 1)));
        CHECK(c.off % A == 0 && c.off >= o + bytes && c.off < o + bytes + A);
        end_of_last = o + bytes;
        prev = c.off;
    }
}

static size_t pad(size_t b) { return (b + 15) & ~(size_t)15; }

enum { B_IN, B_OUT, B_STOP, NB };
enum { IN = 1, OUT = 2, INOUT = 3 };

struct Row {  // one declaration of an entry point
    int buf;
    size_t elem, rows, width;
    int dir;
    bool null;  // the caller passed no array
};
struct Copy {
    int dir, buf;
    size_t off, bytes;
    const void *host;
    bool operator==(const Copy &o) const { return dir == o.dir && buf == o.buf && off == o.off && bytes == o.bytes && host == o.host; }
};

struct RecordingWs {
    std::vector<char> dev[NB];
    std::vector<Copy> log;
    void upload(int buf, const void *src, size_t bytes, size_t off)
    {
        std::memcpy(dev[buf].data() + off, src, bytes);
        log.push_back({IN, buf, off, bytes, src});
    }
    void download(void *dst, int buf, size_t bytes, size_t off)
    {
        std::memcpy(dst, dev[buf].data() + off, bytes);
        log.push_back({OUT, buf, off, bytes, dst});
    }
};

template <typename T> static size_t declare(HostPlan<NB> &plan, const Row &r, char *host, size_t width)
{
    T *h = reinterpret_cast<T *>(host);
    return (r.dir == IN ? plan.in(r.buf, h, r.rows, width) : r.dir == OUT ? plan.out(r.buf, h, r.rows, width) : plan.inout(r.buf, h, r.rows, width)).off;
}

// One call of an entry point: `rows` its declarations; `offsets` (one per row) and `block` (one per buffer) by hand; `want`
// the copies its guards allowed, uploads then downloads, each naming its row in `host` (filled in here).
static void run(const std::vector<Row> &rows, const std::vector<size_t> &offsets, const size_t (&block)[NB], std::vector<Copy> want,
                const std::vector<int> &want_row)
{
    CHECK(rows.size() == offsets.size() && want.size() == want_row.size());
    std::vector<char *> host;
    HostPlan<NB> plan;
    for (size_t i = 0; i < rows.size(); i++) {
        const Row &r = rows[i];
        const size_t bytes = r.rows * r.width * r.elem;
        host.push_back(r.null ? nullptr : new char[bytes]);  // bytes == 0: a real pointer to nothing
        if (host[i])
            std::memset(host[i], (int)(i + 1), bytes);
        size_t off;
        switch (r.elem) {
        case 1: off = declare<uint8_t>(plan, r, host[i], r.width); break;
        case 4: off = declare<uint32_t>(plan, r, host[i], r.width); break;
        case 8: off = declare<uint64_t>(plan, r, host[i], r.width); break;
        default: CHECK(r.rows == 1 && r.width == 1); off = declare<uint8_t>(plan, r, host[i], r.elem);  // a result struct
        }
        CHECK(off == offsets[i] && off % 16 == 0);
    }
    CHECK(plan.ok());
    RecordingWs ws;
    for (int b = 0; b < NB; b++) {
        CHECK(plan.bytes(b) == block[b]);
        ws.dev[b].assign(plan.bytes(b), 0);
    }
    plan.upload(ws);
    const size_t n_up = ws.log.size();
    plan.download(ws);
    for (size_t i = 0; i < want.size(); i++)
        want[i].host = host[want_row[i]];
    CHECK(ws.log.size() == want.size());
    for (size_t i = 0; i < want.size(); i++) {
        CHECK(ws.log[i] == want[i]);
        CHECK((i < n_up) == (want[i].dir == IN));
    }
    for (size_t i = 0; i < rows.size(); i++) {  // what went up came back: every in/out array is what it was
        const size_t bytes = rows[i].rows * rows[i].width * rows[i].elem;
        for (size_t k = 0; host[i] && rows[i].dir == INOUT && k < bytes; k++)
            CHECK(host[i][k] == (char)(i + 1));
        delete[] host[i];
    }
}

// Collects the copies the parent's guards allowed.
struct Want {
    std::vector<Copy> copies;
    std::vector<int> row;
    void up(bool guard, int buf, size_t off, size_t bytes, int r) { add(guard, IN, buf, off, bytes, r); }
    void down(bool guard, int buf, size_t off, size_t bytes, int r) { add(guard, OUT, buf, off, bytes, r); }
    void add(bool guard, int dir, int buf, size_t off, size_t bytes, int r)
    {
        if (guard)
            copies.push_back({dir, buf, off, bytes, nullptr}), row.push_back(r);
    }
};

// opt: every optional output given.  all: the *_all flavour.
static void sim3(int n1, int H, bool all, bool opt)
{
    const size_t words = (size_t)(n1 + 63) / 64, c1 = (size_t)std::max(n1, 1), cH = (size_t)std::max(H, 1);
    const size_t i_valid = 0, i_x1 = i_valid + pad(c1), i_x2 = i_x1 + pad(12 * c1), i_o1 = i_x2 + pad(12 * c1),
                 i_o2 = i_o1 + pad(4 * c1), i_tr = i_o2 + pad(4 * c1), in_bytes = i_tr + pad(12 * cH);
    const size_t o_res = 0, o_cnt = o_res + pad(sizeof(orbgpu_sim3_result)), o_R = o_cnt + pad(4 * cH), o_t = o_R + pad(36 * cH),
                 o_s = o_t + pad(12 * cH), o_T = o_s + pad(4 * cH), o_m = o_T + pad(64 * cH),
                 out_bytes = o_m + pad(8 * cH * std::max<size_t>(words, 1));
    const size_t N1 = (size_t)n1, h = (size_t)H;
    const bool big = all && opt;  // R / t / s / T12 / masks are fetched whole by the *_all flavour only
    const std::vector<Row> rows = {{B_IN, 1, N1, 1, IN, false},  {B_IN, 4, N1, 3, IN, false}, {B_IN, 4, N1, 3, IN, false},
                                   {B_IN, 4, N1, 1, IN, false},  {B_IN, 4, N1, 1, IN, false}, {B_IN, 4, h, 3, IN, false},
                                   {B_OUT, sizeof(orbgpu_sim3_result), 1, 1, OUT, false},     {B_OUT, 4, h, 1, OUT, !opt},
                                   {B_OUT, 4, h, 9, OUT, !big},  {B_OUT, 4, h, 3, OUT, !big}, {B_OUT, 4, h, 1, OUT, !big},
                                   {B_OUT, 4, h, 16, OUT, !big}, {B_OUT, 8, h, words, OUT, !big}};
    Want w;
    w.up(n1 > 0, B_IN, i_valid, N1, 0), w.up(n1 > 0, B_IN, i_x1, 12 * N1, 1), w.up(n1 > 0, B_IN, i_x2, 12 * N1, 2);
    w.up(n1 > 0, B_IN, i_o1, 4 * N1, 3), w.up(n1 > 0, B_IN, i_o2, 4 * N1, 4), w.up(H > 0, B_IN, i_tr, 12 * h, 5);
    w.down(true, B_OUT, o_res, sizeof(orbgpu_sim3_result), 6), w.down(opt && H > 0, B_OUT, o_cnt, 4 * h, 7);
    w.down(big && H > 0, B_OUT, o_R, 36 * h, 8), w.down(big && H > 0, B_OUT, o_t, 12 * h, 9);
    w.down(big && H > 0, B_OUT, o_s, 4 * h, 10), w.down(big && H > 0, B_OUT, o_T, 64 * h, 11);
    w.down(big && H > 0 && words > 0, B_OUT, o_m, 8 * words * h, 12);
    run(rows, {i_valid, i_x1, i_x2, i_o1, i_o2, i_tr, o_res, o_cnt, o_R, o_t, o_s, o_T, o_m}, {in_bytes, out_bytes, 0}, w.copies, w.row);
}

// The downloads in declaration order: the entry point fetched the returned mask's words before Tcw.
static void pnp(int n1, int H, int ms, bool all, bool opt)
{
    const size_t words = (size_t)(n1 + 63) / 64, c1 = (size_t)std::max(n1, 1), cH = (size_t)std::max(H, 1), w1 = std::max<size_t>(words, 1);
    const size_t i_valid = 0, i_x = i_valid + pad(c1), i_kp = i_x + pad(12 * c1), i_o = i_kp + pad(8 * c1), i_s = i_o + pad(4 * c1),
                 in_bytes = i_s + pad(4 * cH * (size_t)ms);
    const size_t o_res = 0, o_cnt = o_res + pad(sizeof(orbgpu_pnp_result)), o_T = o_cnt + pad(4 * cH), o_rm = o_T + pad(64 * cH),
                 o_m = o_rm + pad(8 * w1), out_bytes = o_m + pad(8 * cH * w1);
    const size_t N1 = (size_t)n1, h = (size_t)H;
    const bool big = all && opt;
    const std::vector<Row> rows = {{B_IN, 1, N1, 1, IN, false}, {B_IN, 4, N1, 3, IN, false}, {B_IN, 4, N1, 2, IN, false},
                                   {B_IN, 4, N1, 1, IN, false}, {B_IN, 4, h, (size_t)ms, IN, false},
                                   {B_OUT, sizeof(orbgpu_pnp_result), 1, 1, OUT, false}, {B_OUT, 4, h, 1, OUT, !opt},
                                   {B_OUT, 4, h, 16, OUT, !big}, {B_OUT, 8, 1, words, OUT, false}, {B_OUT, 8, h, words, OUT, !big}};
    Want w;
    w.up(n1 > 0, B_IN, i_valid, N1, 0), w.up(n1 > 0, B_IN, i_x, 12 * N1, 1), w.up(n1 > 0, B_IN, i_kp, 8 * N1, 2);
    w.up(n1 > 0, B_IN, i_o, 4 * N1, 3), w.up(H > 0, B_IN, i_s, 4 * h * (size_t)ms, 4);
    w.down(true, B_OUT, o_res, sizeof(orbgpu_pnp_result), 5), w.down(opt && H > 0, B_OUT, o_cnt, 4 * h, 6);
    w.down(big && H > 0, B_OUT, o_T, 64 * h, 7), w.down(words > 0, B_OUT, o_rm, 8 * words, 8);
    w.down(big && H > 0 && words > 0, B_OUT, o_m, 8 * words * h, 9);
    run(rows, {i_valid, i_x, i_kp, i_o, i_s, o_res, o_cnt, o_T, o_rm, o_m}, {in_bytes, out_bytes, 0}, w.copies, w.row);
}

// inlier may be null only when n1 == 0
static void sim3_opt(int n1, bool opt)
{
    const size_t c1 = (size_t)std::max(n1, 1);
    const size_t i_valid = 0, i_x1 = i_valid + pad(c1), i_x2 = i_x1 + pad(12 * c1), i_o1 = i_x2 + pad(12 * c1),
                 i_o2 = i_o1 + pad(4 * c1), i_k1 = i_o2 + pad(4 * c1), i_k2 = i_k1 + pad(8 * c1), in_bytes = i_k2 + pad(8 * c1);
    const size_t o_res = 0, o_inl = o_res + pad(sizeof(orbgpu_sim3_opt_result)), out_bytes = o_inl + pad(c1);
    const size_t N1 = (size_t)n1;
    const std::vector<Row> rows = {{B_IN, 1, N1, 1, IN, false}, {B_IN, 4, N1, 3, IN, false}, {B_IN, 4, N1, 3, IN, false},
                                   {B_IN, 4, N1, 1, IN, false}, {B_IN, 4, N1, 1, IN, false}, {B_IN, 4, N1, 2, IN, false},
                                   {B_IN, 4, N1, 2, IN, false}, {B_OUT, sizeof(orbgpu_sim3_opt_result), 1, 1, OUT, false},
                                   {B_OUT, 1, N1, 1, INOUT, n1 == 0 && !opt}};
    Want w;
    w.up(n1 > 0, B_IN, i_valid, N1, 0), w.up(n1 > 0, B_IN, i_x1, 12 * N1, 1), w.up(n1 > 0, B_IN, i_x2, 12 * N1, 2);
    w.up(n1 > 0, B_IN, i_o1, 4 * N1, 3), w.up(n1 > 0, B_IN, i_o2, 4 * N1, 4), w.up(n1 > 0, B_IN, i_k1, 8 * N1, 5);
    w.up(n1 > 0, B_IN, i_k2, 8 * N1, 6), w.up(n1 > 0, B_OUT, o_inl, N1, 8);
    w.down(true, B_OUT, o_res, sizeof(orbgpu_sim3_opt_result), 7), w.down(n1 > 0, B_OUT, o_inl, N1, 8);
    run(rows, {i_valid, i_x1, i_x2, i_o1, i_o2, i_k1, i_k2, o_res, o_inl}, {in_bytes, out_bytes, 0}, w.copies, w.row);
}

// The uploads in declaration order: the entry point sent matches12 before kp2.
static void initializer(int n1, int n2, int H, bool all, bool opt)
{
    const size_t words = (size_t)(n1 + 63) / 64, c1 = (size_t)std::max(n1, 1), c2 = (size_t)std::max(n2, 1), cH = (size_t)std::max(H, 1),
                 w1 = std::max<size_t>(words, 1);
    const size_t i_k1 = 0, i_k2 = i_k1 + pad(8 * c1), i_m = i_k2 + pad(8 * c2), i_s = i_m + pad(4 * c1), in_bytes = i_s + pad(32 * cH);
    const size_t o_res = 0, o_p = o_res + pad(sizeof(orbgpu_init_result)), o_t = o_p + pad(12 * c1), o_sh = o_t + pad(c1),
                 o_sf = o_sh + pad(4 * cH), o_mh = o_sf + pad(4 * cH), o_mf = o_mh + pad(8 * cH * w1), out_bytes = o_mf + pad(8 * cH * w1);
    const size_t N1 = (size_t)n1, N2 = (size_t)n2, h = (size_t)H;
    const bool big = all && opt;
    const std::vector<Row> rows = {{B_IN, 4, N1, 2, IN, false}, {B_IN, 4, N2, 2, IN, false}, {B_IN, 4, N1, 1, IN, false},
                                   {B_IN, 4, h, 8, IN, false},  {B_OUT, sizeof(orbgpu_init_result), 1, 1, OUT, false},
                                   {B_OUT, 4, N1, 3, OUT, !opt}, {B_OUT, 1, N1, 1, OUT, !opt}, {B_OUT, 4, h, 1, OUT, !big},
                                   {B_OUT, 4, h, 1, OUT, !big}, {B_OUT, 8, h, words, OUT, !big}, {B_OUT, 8, h, words, OUT, !big}};
    Want w;
    w.up(n1 > 0, B_IN, i_k1, 8 * N1, 0), w.up(n2 > 0, B_IN, i_k2, 8 * N2, 1), w.up(n1 > 0, B_IN, i_m, 4 * N1, 2);
    w.up(H > 0, B_IN, i_s, 32 * h, 3);
    w.down(true, B_OUT, o_res, sizeof(orbgpu_init_result), 4), w.down(opt && n1 > 0, B_OUT, o_p, 12 * N1, 5);
    w.down(opt && n1 > 0, B_OUT, o_t, N1, 6), w.down(big && H > 0, B_OUT, o_sh, 4 * h, 7), w.down(big && H > 0, B_OUT, o_sf, 4 * h, 8);
    w.down(big && H > 0 && words > 0, B_OUT, o_mh, 8 * words * h, 9), w.down(big && H > 0 && words > 0, B_OUT, o_mf, 8 * words * h, 10);
    run(rows, {i_k1, i_k2, i_m, i_s, o_res, o_p, o_t, o_sh, o_sf, o_mh, o_mf}, {in_bytes, out_bytes, 0}, w.copies, w.row);
}

// orbgpu_local_ba: np = n_local, F = n_edges (erase); orbgpu_bundle_adjustment: np = n_poses, F = n_points (not_included).
// opt: Tcw_d and pos_d given.
static void bundle_adjustment(size_t result_bytes, size_t np, size_t M, size_t F, bool opt)
{
    const size_t o_res = 0, o_Td = o_res + pad(result_bytes), o_T = o_Td + pad(128 * std::max<size_t>(np, 1)),
                 o_Xd = o_T + pad(64 * std::max<size_t>(np, 1)), o_X = o_Xd + pad(24 * std::max<size_t>(M, 1)),
                 o_f = o_X + pad(12 * std::max<size_t>(M, 1)), out_bytes = o_f + pad(std::max<size_t>(F, 1));
    const std::vector<Row> rows = {{B_STOP, 4, 1, 1, IN, false},       {B_OUT, result_bytes, 1, 1, OUT, false}, {B_OUT, 8, np, 16, INOUT, !opt},
                                   {B_OUT, 4, np, 16, INOUT, false},   {B_OUT, 8, M, 3, INOUT, !opt},           {B_OUT, 4, M, 3, INOUT, false},
                                   {B_OUT, 1, F, 1, INOUT, false}};
    Want w;
    w.up(true, B_STOP, 0, 4, 0);
    for (int dir : {IN, OUT}) {
        w.down(dir == OUT, B_OUT, o_res, result_bytes, 1);
        w.add(np && opt, dir, B_OUT, o_Td, 128 * np, 2), w.add(np, dir, B_OUT, o_T, 64 * np, 3);
        w.add(M && opt, dir, B_OUT, o_Xd, 24 * M, 4), w.add(M, dir, B_OUT, o_X, 12 * M, 5), w.add(F, dir, B_OUT, o_f, F, 6);
    }
    run(rows, {0, o_res, o_Td, o_T, o_Xd, o_X, o_f}, {0, out_bytes, 16}, w.copies, w.row);
}

// opt: Siw_d given
static void essential_graph(size_t V, size_t M, bool opt)
{
    const size_t i_scw = 0, i_pos = i_scw + pad(64 * std::max<size_t>(V, 1)), i_ref = i_pos + pad(12 * std::max<size_t>(M, 1)),
                 in_bytes = i_ref + pad(4 * std::max<size_t>(M, 1));
    const size_t o_res = 0, o_Sd = o_res + pad(sizeof(orbgpu_essential_graph_result)), o_T = o_Sd + pad(64 * std::max<size_t>(V, 1)),
                 o_X = o_T + pad(64 * std::max<size_t>(V, 1)), out_bytes = o_X + pad(12 * std::max<size_t>(M, 1));
    const std::vector<Row> rows = {{B_STOP, 4, 1, 1, IN, false}, {B_IN, 8, V, 8, IN, false}, {B_IN, 4, M, 3, IN, false}, {B_IN, 4, M, 1, IN, false},
                                   {B_OUT, sizeof(orbgpu_essential_graph_result), 1, 1, OUT, false}, {B_OUT, 8, V, 8, INOUT, !opt},
                                   {B_OUT, 4, V, 16, INOUT, false}, {B_OUT, 4, M, 3, INOUT, false}};
    Want w;
    w.up(true, B_STOP, 0, 4, 0), w.up(V, B_IN, i_scw, 64 * V, 1), w.up(M, B_IN, i_pos, 12 * M, 2), w.up(M, B_IN, i_ref, 4 * M, 3);
    for (int dir : {IN, OUT}) {
        w.down(dir == OUT, B_OUT, o_res, sizeof(orbgpu_essential_graph_result), 4);
        w.add(V && opt, dir, B_OUT, o_Sd, 64 * V, 5), w.add(V, dir, B_OUT, o_T, 64 * V, 6), w.add(M, dir, B_OUT, o_X, 12 * M, 7);
    }
    run(rows, {0, i_scw, i_pos, i_ref, o_res, o_Sd, o_T, o_X}, {in_bytes, out_bytes, 16}, w.copies, w.row);
}

// One copy more than the plan holds: the plan says so (host_begin refuses it), the segment is still carved, and neither the
// records nor anything behind them is written.
static void capacity()
{
    struct {
        HostPlan<1> plan;
        unsigned char guard[64];
    } s;
    std::memset(s.guard, 0xA5, sizeof(s.guard));
    uint32_t v[HostPlan<1>::MAX_SEGS + 1] = {};
    for (int i = 0; i < HostPlan<1>::MAX_SEGS; i++)
        CHECK(s.plan.in(0, &v[i], 1).off == 16 * (size_t)i);
    CHECK(s.plan.ok());
    CHECK(s.plan.out(0, (uint32_t *)nullptr, 1).off == 16 * (size_t)HostPlan<1>::MAX_SEGS);  // nothing to copy: not counted
    CHECK(s.plan.ok());
    CHECK(s.plan.in(0, &v[HostPlan<1>::MAX_SEGS], 1).off == 16 * (size_t)(HostPlan<1>::MAX_SEGS + 1));
    CHECK(!s.plan.ok() && s.plan.bytes(0) == 16 * (size_t)(HostPlan<1>::MAX_SEGS + 2));
    for (unsigned char g : s.guard)
        CHECK(g == 0xA5);
    RecordingWs ws;
    ws.dev[0].assign(s.plan.bytes(0), 0);
    s.plan.upload(ws);
    CHECK(ws.log.size() == (size_t)HostPlan<1>::MAX_SEGS);
}

int main()
{
    sequence(Carver(), 256);  // the default: the id tables' blocks
    sequence(Carver(256), 256);
    sequence(Carver(16), 16);
    for (bool opt : {false, true}) {
        for (int n1 : {0, 1, 15, 16, 17, 64, 65})
            for (int H : {0, 1, 3})
                for (bool all : {false, true}) {
                    sim3(n1, H, all, opt);
                    for (int ms : {4, 5})
                        pnp(n1, H, ms, all, opt);
                    sim3_opt(n1, opt);
                    for (int n2 : {0, 1, 17})
                        initializer(n1, n2, H, all, opt);
                }
        for (size_t np : {0, 1, 3})
            for (size_t M : {0, 1, 5}) {
                for (size_t E : {0, 1, 7})
                    bundle_adjustment(sizeof(orbgpu_local_ba_result), np, M, E, opt);
                bundle_adjustment(sizeof(orbgpu_bundle_adjustment_result), np, M, M, opt);
            }
        for (size_t V : {0, 1, 3})
            for (size_t M : {0, 1, 5})
                essential_graph(V, M, opt);
    }
    capacity();
    std::printf("carve_test ok\n");
    return 0;
}
