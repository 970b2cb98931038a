// The extractor's host-only plan (orb_slam2_map_amd/csrc/extractor_plan.h) without a device:
//   extractor_plan_test W H NFEATURES SCALE NLEVELS QT_KEYS_HOOK
// plans the size, checks the plan's invariants and prints
//   "D <name> <value>"  every scalar of the plan, and a field-wise FNV-1a digest of every table (the golden file)
//   "L <level> <w> <h> <quota> <sel_cap>"  what tests/test_extractor_plan.py compares with the oracle
// then "extractor_plan_test ok".  A refused size prints "refused: <reason>" and exits with 3.
#include "extractor_plan.h"

#include <cinttypes>

using namespace orbgpu;

#define CHECK(cond, ...)                                    \
    do {                                                    \
        if (!(cond)) {                                      \
            printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); \
            printf(__VA_ARGS__);                            \
            printf("\n");                                   \
            exit(1);                                        \
        }                                                   \
    } while (0)

// ---- digests --------------------------------------------------------------------------------------------------------
static uint64_t fnv(const void *first, size_t stride, size_t size, size_t n)
{
    uint64_t hsh = 1469598103934665603ull;
    for (size_t i = 0; i < n; i++)
        for (size_t b = 0; b < size; b++)
            hsh = (hsh ^ static_cast<const uint8_t *>(first)[i * stride + b]) * 1099511628211ull;
    return hsh;
}
#define DIG(name, arr, n, field)                                                                                   \
    printf("D " name "." #field " %zu:%016" PRIx64 "\n", (size_t)(n),                                             \
           fnv((n) ? (const void *)&(arr)[0].field : nullptr, sizeof((arr)[0]), sizeof((arr)[0].field), (n)))
#define DIGRAW(name, arr, n) \
    printf("D " name " %zu:%016" PRIx64 "\n", (size_t)(n), fnv((n) ? (const void *)(arr) : nullptr, sizeof((arr)[0]), sizeof((arr)[0]), (n)))
#define VAL(name, v) printf("D " name " %lld\n", (long long)(v))

struct PlanView {  // what is digested, by pointer: the same text digests any holder of these tables
    int nl;
    const float *scale, *inv_scale, *sigma2, *inv_sigma2;
    const int *quota, *umax;
    const LevelGeom *geom;
    const CellDesc *cells; size_t ncells;
    const ColumnInfo *ctab; size_t nctab;
    const BorderCol *bcol; size_t nbcol;
    const XTab *xtab; size_t nxtab;
    const YTab *ytab; size_t nytab;
    const YRow *yrow; size_t nyrow;
    const ResizeStrip *rstrip; size_t nrstrip;
    const RsQuad *rsel, *rwt; size_t nrsel, nrwt;
    const uint32_t *r8item; size_t nr8item;
    const RsQuad *r8sel, *r8wt; size_t nr8sel, nr8wt;
    const uint32_t *orw; size_t norw;
    const StripGeom *blur;
    const DetectGeom *det, *detd;
    long long frame_pyr, frame_slots, sel_cap_total, ncap, max_kp, qt_lds, qt_kcap, max_slots_level, qt_prefilter, border_fast,
        direct0_ok, rs_off_direct, r8_off_direct, r8_share_direct, interior_resize;
    const int *r8_off;
    const bool *r8_share;
};

static void dump_view(const PlanView &v)
{
    const size_t nl = (size_t)v.nl;
    VAL("nlevels", v.nl);
    DIGRAW("consts.scale", v.scale, nl);
    DIGRAW("consts.inv_scale", v.inv_scale, nl);
    DIGRAW("consts.sigma2", v.sigma2, nl);
    DIGRAW("consts.inv_sigma2", v.inv_sigma2, nl);
    DIGRAW("consts.quota", v.quota, nl);
    DIGRAW("consts.umax", v.umax, (size_t)16);
#define G(f) DIG("geom", v.geom, nl, f)
    G(w); G(h); G(pitch); G(plane_off); G(max_bx); G(max_by); G(ncols); G(nrows); G(wcell); G(hcell); G(cell_first); G(ncells);
    G(slot_off); G(slot_cnt); G(quota); G(sel_cap); G(sel_off); G(n_ini); G(hx); G(scale); G(patch); G(xtab_off); G(ytab_off);
    G(rs_off); G(rs_fast); G(ncols_eff); G(inv_wcell); G(inv_hcell); G(yrow_off);
#undef G
#define C(f) DIG("cells", v.cells, v.ncells, f)
    C(level); C(x0); C(y0); C(x1); C(y1); C(addx); C(addy); C(cap); C(slot_off); C(pitch); C(plane_off); C(pad);
#undef C
    DIG("ctab", v.ctab, v.nctab, cellj);
    DIG("ctab", v.ctab, v.nctab, flags);
    DIG("bcol", v.bcol, v.nbcol, d);
    DIG("bcol", v.bcol, v.nbcol, sel);
    DIG("xtab", v.xtab, v.nxtab, sx); DIG("xtab", v.xtab, v.nxtab, sx1); DIG("xtab", v.xtab, v.nxtab, a0); DIG("xtab", v.xtab, v.nxtab, a1);
    DIG("ytab", v.ytab, v.nytab, sy0); DIG("ytab", v.ytab, v.nytab, sy1); DIG("ytab", v.ytab, v.nytab, b0); DIG("ytab", v.ytab, v.nytab, b1);
    DIG("yrow", v.yrow, v.nyrow, sy0); DIG("yrow", v.yrow, v.nyrow, sy1); DIG("yrow", v.yrow, v.nyrow, b0); DIG("yrow", v.yrow, v.nyrow, b1);
    DIG("rstrip", v.rstrip, v.nrstrip, base_q);
    DIGRAW("rsel", v.rsel, v.nrsel);
    DIGRAW("rwt", v.rwt, v.nrwt);
    DIGRAW("r8item", v.r8item, v.nr8item);
    DIGRAW("r8sel", v.r8sel, v.nr8sel);
    DIGRAW("r8wt", v.r8wt, v.nr8wt);
    DIGRAW("orient", v.orw, v.norw);
    const size_t one = 1;
    DIG("blur", v.blur, one, first); DIG("blur", v.blur, one, nsx); DIG("blur", v.blur, one, nlevels);
    DIG("det", v.det, one, first); DIG("det", v.det, one, nsx); DIG("det", v.det, one, ncols); DIG("det", v.det, one, ctab_off);
    DIG("det", v.det, one, xfirst); DIG("det", v.det, one, nlevels);
    DIG("detd", v.detd, one, first); DIG("detd", v.detd, one, nsx); DIG("detd", v.detd, one, ncols); DIG("detd", v.detd, one, ctab_off);
    DIG("detd", v.detd, one, xfirst); DIG("detd", v.detd, one, nlevels);
    VAL("frame_pyr", v.frame_pyr); VAL("frame_slots", v.frame_slots); VAL("sel_cap_total", v.sel_cap_total); VAL("ncap", v.ncap);
    VAL("max_kp", v.max_kp); VAL("qt_lds", v.qt_lds); VAL("qt_kcap", v.qt_kcap); VAL("max_slots_level", v.max_slots_level);
    VAL("qt_prefilter", v.qt_prefilter); VAL("border_fast", v.border_fast); VAL("direct0_ok", v.direct0_ok);
    VAL("rs_off_direct", v.rs_off_direct); VAL("r8_off_direct", v.r8_off_direct); VAL("r8_share_direct", v.r8_share_direct);
    VAL("interior_resize", v.interior_resize);
    DIGRAW("r8_off", v.r8_off, (size_t)ORBGPU_MAX_LEVELS);
    DIGRAW("r8_share", v.r8_share, (size_t)ORBGPU_MAX_LEVELS);
}

// ---- invariants -----------------------------------------------------------------------------------------------------
static void check_detect(const ExtractorPlan &P, const DetectGeom &d, bool direct0)
{
    const int nl = (int)P.geom.size();
    const ColumnInfo *ctab = P.table<ColumnInfo>(P.t_ctab);
    std::vector<int> lo_of, hi_of;  // per flat strip: the cell ids its four pixels touch
    CHECK(d.nlevels == nl, "%d", d.nlevels);
    for (int l = 0; l < nl; l++) {
        const LevelGeom &g = P.geom[l];
        const int xfirst = d.xfirst[l], nbands = (g.h - 2 * EDGE + g.hcell - 1) / g.hcell;
        CHECK(xfirst == (direct0 && l == 0 ? 16 : 17) && d.ncols[l] == g.ncols_eff, "level %d", l);
        CHECK(xfirst + 4 * d.nsx[l] - 1 >= g.w - 20, "level %d: strips end before the last scored column", l);
        CHECK(d.first[l] >= (int)lo_of.size() && d.first[l + 1] >= d.first[l] + d.nsx[l] * nbands, "level %d", l);
        CHECK(d.ctab_off[l] >= 0 && (size_t)(d.ctab_off[l] + d.nsx[l]) <= P.count<ColumnInfo>(P.t_ctab), "level %d", l);
        lo_of.resize((size_t)d.first[l], -1);
        hi_of.resize((size_t)d.first[l], -1);
        for (int b = 0; b < nbands; b++)
            for (int sx = 0; sx < d.nsx[l]; sx++) {
                const ColumnInfo &c = ctab[d.ctab_off[l] + sx];
                int lo = -1, hi = -1;
                for (int p = 0; p < 4; p++) {
                    // a column belongs to cell column (x - EDGE) / wcell when it is inside the image interior and that cell
                    // column is not one the reference skips
                    const int x = xfirst + 4 * sx + p;
                    const int j = x >= EDGE ? (x - EDGE) / g.wcell : -1;
                    const bool valid = x >= EDGE && x < g.w - EDGE && j < g.ncols_eff;
                    const bool first = valid && (x - EDGE) % g.wcell == 0;
                    const bool last = valid && (x == g.w - EDGE - 1 || (x - EDGE) % g.wcell == g.wcell - 1);
                    CHECK((int)((c.cellj >> (8 * p)) & 255u) == (valid ? j : 0xFF), "level %d column %d", l, x);
                    CHECK((((c.flags >> p) & 1u) != 0) == valid && (((c.flags >> (4 + p)) & 1u) != 0) == first &&
                              (((c.flags >> (8 + p)) & 1u) != 0) == last, "level %d column %d flags %x", l, x, c.flags);
                    if (valid) {
                        const int id = g.cell_first + b * g.ncols_eff + j;
                        CHECK(id < g.cell_first + g.ncells, "level %d band %d: cell %d", l, b, id);
                        lo = lo < 0 ? id : std::min(lo, id);
                        hi = std::max(hi, id);
                    }
                }
                lo_of.push_back(lo);
                hi_of.push_back(hi);
            }
    }
    for (size_t w0 = 0; w0 < lo_of.size(); w0 += FD_OWN) {
        int lo = 1 << 30, hi = -1;
        for (size_t q = w0; q < std::min(w0 + FD_OWN, lo_of.size()); q++)
            if (lo_of[q] >= 0) {
                lo = std::min(lo, lo_of[q]);
                hi = std::max(hi, hi_of[q]);
            }
        CHECK(hi < 0 || hi - lo < FD_CELLS, "wave %zu spans cells %d..%d", w0 / FD_OWN, lo, hi);
    }
}

static void check_plan(const ExtractorConsts &cst, const ExtractorPlan &P, int w, int h, int qt_keys)
{
    const int nl = cst.nlevels;
    CHECK(P.w == w && P.h == h && (int)P.geom.size() == nl, "size");
    // (2) slots of the cells: contiguous, disjoint, frame_slots in all; (10) max_keypoints' helpers give the plan's caps
    const CellDesc *cells = P.table<CellDesc>(P.t_cells);
    CHECK(P.count<CellDesc>(P.t_cells) == (size_t)P.ncells, "cells");
    int slot = 0, cell = 0, sel = 0, max_kp = 0;
    for (int l = 0; l < nl; l++) {
        const LevelGeom &g = P.geom[l];
        CHECK(g.cell_first == cell && g.slot_off == slot && g.ncells > 0, "level %d", l);
        for (int i = 0; i < g.ncells; i++, cell++) {
            CHECK(cells[cell].level == l && cells[cell].slot_off == slot && cells[cell].cap >= 0, "cell %d", cell);
            CHECK(cells[cell].pitch == g.pitch && cells[cell].plane_off == g.plane_off, "cell %d", cell);
            slot += cells[cell].cap;
        }
        CHECK(g.slot_cnt == slot - g.slot_off && g.slot_cnt <= P.max_slots_level, "level %d", l);
        // (3) selection slots
        CHECK(g.sel_off == sel && g.sel_cap <= P.ncap, "level %d", l);
        sel += g.sel_cap;
        max_kp += g.sel_cap - 1;
        const LevelSize ls = level_size(cst, w, h, l);
        CHECK(ls.w == g.w && ls.h == g.h && level_n_ini(ls) == g.n_ini, "level %d", l);
        CHECK(level_max_keypoints(level_n_ini(ls), cst.quota[l]) + 1 == g.sel_cap, "level %d", l);
        // (6) the reciprocals divide exactly
        for (uint32_t v = 0; v < 8192u; v++)
            CHECK((uint32_t)(((uint64_t)v * g.inv_wcell) >> 32) == v / (uint32_t)g.wcell &&
                      (uint32_t)(((uint64_t)v * g.inv_hcell) >> 32) == v / (uint32_t)g.hcell, "level %d v %u", l, v);
        // (8) blur strips: 8 bytes each from padded byte 16, down to the last row
        CHECK(16 + 8 * P.blur_geom.nsx[l] > EDGE + g.w - 1, "level %d: blur strips stop before column w-1", l);
        CHECK(P.blur_geom.first[l + 1] - P.blur_geom.first[l] == P.blur_geom.nsx[l] * ((g.h + BLUR_ROWS - 1) / BLUR_ROWS), "level %d", l);
        CHECK(16 + 8 * P.blur_geom.nsx[l] <= g.pitch, "level %d: blur strips leave the row", l);
    }
    CHECK(cell == P.ncells && (size_t)slot == P.frame_slots, "%d cells, %d slots", cell, slot);
    CHECK(sel == P.sel_cap_total && max_kp == P.max_kp && P.ncap % 8 == 0, "%d %d", sel, max_kp);
    // (4), (5) the column tables of k_fast_detect
    check_detect(P, P.det_geom, false);
    if (P.direct0_ok)
        check_detect(P, P.det_geom_direct, true);
    CHECK(!P.direct0_ok || (w % 8 == 0 && nl >= 2), "direct mode");
    // (7) level-0 border columns
    const BorderCol *bcol = P.table<BorderCol>(P.t_bcol);
    CHECK(P.border_fast == (w % 4 == 0) && P.count<BorderCol>(P.t_bcol) == (P.border_fast ? (size_t)P.geom[0].pitch / 4 : 0), "bcol");
    for (size_t c = 0; c < P.count<BorderCol>(P.t_bcol); c++)
        for (int k = 0; k < 4; k++) {
            const int idx = (int)((bcol[c].sel >> (8 * k)) & 255u);
            CHECK(idx < 8 && (int)bcol[c].d * 4 + 8 <= w, "column %zu", c);
            CHECK((int)bcol[c].d * 4 + idx == reflect101(std::min((int)c * 4 + k, w + 2 * EDGE - 1) - EDGE, w), "column %zu byte %d", c, k);
        }
    // (9) the arena
    const PlanTable *tabs[] = {&P.t_geom, &P.t_cells, &P.t_ctab, &P.t_bcol, &P.t_xtab, &P.t_ytab, &P.t_yrow, &P.t_rstrip, &P.t_rsel,
                               &P.t_rwt, &P.t_r8item, &P.t_r8sel, &P.t_r8wt, &P.t_pattern, &P.t_orient};
    size_t end = 0;
    for (const PlanTable *t : tabs) {
        CHECK(t->off % PLAN_ALIGN == 0 && t->off >= end && t->off + t->bytes <= P.blob.size(), "table at %zu + %zu", t->off, t->bytes);
        end = t->off + t->bytes;
    }
    CHECK(P.t_geom.bytes == sizeof(LevelGeom) * nl && memcmp(P.table<LevelGeom>(P.t_geom), P.geom.data(), P.t_geom.bytes) == 0, "geom");
    CHECK(P.t_pattern.bytes == 1024 && P.t_orient.bytes == 2 * 4 * 16 * 9 * 4, "pattern");
    CHECK((nl == 1) == (P.t_xtab.bytes == 0) && (nl == 1) == (P.t_yrow.bytes == 0), "resize tables of a single level");
    CHECK(P.t_rsel.bytes == P.t_rstrip.bytes * 4 && P.t_rwt.bytes == P.t_rsel.bytes, "4-pixel tables");
    CHECK(P.t_r8sel.bytes == P.t_r8item.bytes * 8 && P.t_r8wt.bytes == P.t_r8sel.bytes, "8-pixel tables");
    // the launch decisions
    const QuadtreeLaunch q1 = quadtree_launch(P, 1, false), qb = quadtree_launch(P, QT_BATCH_MIN, false), qf = quadtree_launch(P, 1, true);
    CHECK(q1.lds_keys && q1.kcap == P.qt_kcap && q1.lds_bytes == P.qt_lds + 6 * (size_t)P.qt_kcap && q1.lds_bytes <= (size_t)QT_LDS_MAX, "single");
    CHECK(q1.threads == (w * h >= QT_LARGE_PIXELS ? QT_THREADS : QT_THREADS_SMALL), "threads");
    CHECK(!qb.lds_keys && qb.kcap == 0 && qb.threads == QT_THREADS_BATCH && qb.lds_bytes == P.qt_lds, "batch");
    CHECK(!qf.lds_keys && qf.threads == QT_THREADS_BATCH, "forced batch variant");
    CHECK(qt_keys < 0 ? P.qt_kcap >= std::min(P.max_slots_level, 1) : P.qt_kcap == (qt_keys + 7) / 8 * 8, "qt_kcap %d", P.qt_kcap);
    for (int l = 1; l < nl; l++)
        for (int direct = 0; direct <= (P.direct0_ok ? 1 : 0); direct++) {
            const ResizeLaunch r1 = resize_launch(P, l, 1, direct != 0), rb = resize_launch(P, l, PYR_BATCH_MIN, direct != 0);
            const bool dir1 = direct && l == 1;
            const int r8 = dir1 ? P.r8_off_direct : P.r8_off[l];
            CHECK(r1.px == (P.geom[l].rs_fast ? 4 : 0) && rb.px == (!P.geom[l].rs_fast ? 0 : r8 >= 0 ? 8 : 4), "level %d", l);
            CHECK(rb.px == 0 || (rb.rows == PYR_ROWS && rb.dir1 == dir1), "level %d", l);
            CHECK(r1.px == 0 || (r1.off == (dir1 ? P.rs_off_direct : P.geom[l].rs_off) && (r1.rows == 8 || r1.rows == 4 || r1.rows == 2)), "level %d", l);
            CHECK(rb.px != 8 || (rb.off == r8 && (size_t)(r8 + resize_n8(P.geom[l].w)) <= P.count<uint32_t>(P.t_r8item)), "level %d", l);
        }
    CHECK(P.ring_full.nlevels == nl && P.ring_full.first[1] == 0, "ring");
}

int main(int argc, char **argv)
{
    if (argc != 7) {
        printf("usage: %s W H NFEATURES SCALE NLEVELS QT_KEYS_HOOK\n", argv[0]);
        return 2;
    }
    const int w = atoi(argv[1]), h = atoi(argv[2]), nfeatures = atoi(argv[3]), nl = atoi(argv[5]);
    const float sf = (float)atof(argv[4]);
    PlanHooks hooks;
    hooks.qt_keys = atoi(argv[6]);
    ExtractorConsts cst;
    ExtractorPlan P;
    std::string why;
    if (build_consts(nfeatures, sf, nl, &cst, &why) != ORBGPU_OK || plan_extractor(cst, w, h, hooks, &P, &why) != ORBGPU_OK) {
        printf("refused: %s\n", why.c_str());
        return 3;
    }
    check_plan(cst, P, w, h, hooks.qt_keys);
    PlanView v = {};
    v.nl = nl;
    v.scale = cst.scale; v.inv_scale = cst.inv_scale; v.sigma2 = cst.sigma2; v.inv_sigma2 = cst.inv_sigma2;
    v.quota = cst.quota; v.umax = cst.umax.v;
    v.geom = P.geom.data();
#define TAB(T, ptr, cnt, t) v.ptr = P.table<T>(P.t); v.cnt = P.count<T>(P.t)
    TAB(CellDesc, cells, ncells, t_cells); TAB(ColumnInfo, ctab, nctab, t_ctab); TAB(BorderCol, bcol, nbcol, t_bcol);
    TAB(XTab, xtab, nxtab, t_xtab); TAB(YTab, ytab, nytab, t_ytab); TAB(YRow, yrow, nyrow, t_yrow);
    TAB(ResizeStrip, rstrip, nrstrip, t_rstrip); TAB(RsQuad, rsel, nrsel, t_rsel); TAB(RsQuad, rwt, nrwt, t_rwt);
    TAB(uint32_t, r8item, nr8item, t_r8item); TAB(RsQuad, r8sel, nr8sel, t_r8sel); TAB(RsQuad, r8wt, nr8wt, t_r8wt);
    TAB(uint32_t, orw, norw, t_orient);
#undef TAB
    v.blur = &P.blur_geom; v.det = &P.det_geom; v.detd = &P.det_geom_direct;
    v.frame_pyr = (long long)P.frame_pyr; v.frame_slots = (long long)P.frame_slots; v.sel_cap_total = P.sel_cap_total; v.ncap = P.ncap;
    v.max_kp = P.max_kp; v.qt_lds = (long long)P.qt_lds; v.qt_kcap = P.qt_kcap; v.max_slots_level = P.max_slots_level;
    v.qt_prefilter = P.qt_prefilter; v.border_fast = P.border_fast; v.direct0_ok = P.direct0_ok; v.rs_off_direct = P.rs_off_direct;
    v.r8_off_direct = P.r8_off_direct; v.r8_share_direct = P.r8_share_direct; v.interior_resize = P.interior_resize;
    v.r8_off = P.r8_off; v.r8_share = P.r8_share;
    dump_view(v);
    for (int l = 0; l < nl; l++)
        printf("L %d %d %d %d %d\n", l, P.geom[l].w, P.geom[l].h, P.geom[l].quota, P.geom[l].sel_cap);
    for (int l = 0; l < nl; l++)
        printf("C %d %.9g %.9g %.9g %.9g\n", l, cst.scale[l], cst.inv_scale[l], cst.sigma2[l], cst.inv_sigma2[l]);
    printf("A %zu bytes of tables\n", P.blob.size());
    printf("U");
    for (int v0 = 0; v0 < 16; v0++)
        printf(" %d", cst.umax.v[v0]);
    printf("\nextractor_plan_test ok\n");
    return 0;
}
