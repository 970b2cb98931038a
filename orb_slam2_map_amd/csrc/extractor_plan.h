// Host side of the extractor's geometry (extractor.hip): the structs its kernels read, the constructor tables of an
// extractor (ExtractorConsts), everything one image size derives from them (ExtractorPlan: level sizes, FAST cell grid,
// slot layout, strip tables, resize tables, quadtree LDS sizing, and ONE byte blob that holds every constant table the
// kernels read), and the launch decisions that depend on the batch size.  Host-only, no HIP: compiles with plain
// g++ -std=c++17 (tests/extractor_plan_test.cpp), so a plan and its refusals can be checked without a device.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "orbgpu.h"
#include "resize_tables.h"

#ifdef __HIPCC__
#define ORBGPU_PLAN_HD __host__ __device__ __forceinline__
#else
#define ORBGPU_PLAN_HD inline
#endif

namespace orbgpu {

constexpr int EDGE = 19;           // EDGE_THRESHOLD, ORBextractor.cc:74
static_assert(EDGE == RS_EDGE, "resize_tables.h builds its tables for this border");
constexpr int BORDER0 = EDGE - 3;  // minBorderX/Y, ORBextractor.cc:775-776
constexpr int HALF_PATCH = 15;     // HALF_PATCH_SIZE, ORBextractor.cc:73
constexpr int PATCH = 31;          // PATCH_SIZE
constexpr float CELL_W = 30.f;     // W, ORBextractor.cc:769
constexpr int MAX_CELL = 66;       // max cell interior edge

constexpr int PYR_ROWS = 8;        // padded rows per thread in the pyramid kernels
constexpr int PYR_BATCH_MIN = 32;  // frames per call from which every level of the resize chain runs PYR_ROWS rows per item (REUSE)
constexpr int BLUR_ROWS = 30;      // output rows per strip (5 x 6: the 6-slot register ring of row pairs unrolls evenly)

constexpr int FD_OWN = 62;    // columns a wave owns (lanes 1..62)
constexpr int FD_CELLS = 32;  // cells a wave's 64 columns can touch (consecutive ids)

// workgroup size of k_quadtree: a single frame is bound by the latency of its level-0 workgroup (more threads per
// key loop help), a full batch by barrier cost and workgroups per CU (fewer threads help): 155 -> 122 us at B = 256
constexpr int QT_THREADS = 1024, QT_THREADS_SMALL = 512, QT_THREADS_BATCH = 256, QT_BATCH_MIN = 32;
constexpr int QT_LARGE_PIXELS = 700000;  // single frames from about 1024x768 use QT_THREADS (measured: 137 -> 128 us at 1280x960, 51 -> 54 us at 640x480)
constexpr int QT_LDS_MAX = 160 * 1024 - 1024;  // dynamic LDS k_quadtree may be launched with (the CU has 160 KB)
constexpr int QT_INI_MAX = 80;                 // initial nodes of a level k_qt_prefilter supports (round(width / height))

// ---------------------------------------------------------------------------------------------
// Geometry tables (host-built, device-read)
// ---------------------------------------------------------------------------------------------
struct LevelGeom {
    int w, h, pitch;     // level size; padded row pitch in bytes (multiple of 64)
    int plane_off;       // byte offset of the padded plane inside one frame's pyramid block
    int max_bx, max_by;  // maxBorderX/Y = w-16, h-16
    int ncols, nrows, wcell, hcell;
    int cell_first, ncells;  // this level's (non-skipped) cells in the cell table
    int slot_off, slot_cnt;  // this level's key slots inside one frame's slot block (u32 units)
    int quota, sel_cap, sel_off;
    int n_ini;
    float hx;
    float scale;
    int patch;
    int xtab_off, ytab_off;  // resize tables (levels >= 1)
    int rs_off, rs_fast;     // fast-path strip tables (k_resize_fast); rs_fast = 0 -> k_resize_level
    int ncols_eff;           // cell columns that are not skipped (ORBextractor.cc:797)
    uint32_t inv_wcell, inv_hcell;  // mul_hi(v, inv) == v / wcell (hcell) for every key coordinate (host-verified)
    int yrow_off;                   // k_resize_fast: first YRow of the level (one per PADDED output row)
};
static_assert(sizeof(LevelGeom) == 116, "LevelGeom is an array the kernels index");

struct CellDesc {
    short level;
    short x0, y0, x1, y1;  // sub-image [x0,x1) x [y0,y1) in level coordinates (FAST apron included)
    short addx, addy;      // j*wCell, i*hCell  (ORBextractor.cc:822-823)
    short cap;             // slot capacity
    int slot_off;          // offset of this cell's slots inside one frame's slot block
    int pitch, plane_off;  // copies of the level's LevelGeom fields
    int pad[1];
};
static_assert(sizeof(CellDesc) == 32, "CellDesc is read as two 16-byte words");

struct BorderCol {  // k_border0_fast, per aligned dword of the padded level-0 row
    uint32_t d;    // first of the two adjacent source dwords
    uint32_t sel;  // v_perm_b32 selector over {src[d+1], src[d]}
};
static_assert(sizeof(BorderCol) == 8, "BorderCol is read as one 8-byte word");

struct RingGeom {  // k_ring_fill
    int first[ORBGPU_MAX_LEVELS + 1];  // first item of level l (first[1] = 0); first[nlevels] = items per frame
    int nlevels;
};
static_assert(sizeof(RingGeom) == 4 * (ORBGPU_MAX_LEVELS + 2), "RingGeom is a kernel argument");

struct StripGeom {  // strips of all levels, flattened (k_blur)
    int first[ORBGPU_MAX_LEVELS + 1];  // first strip index of each level
    int nsx[ORBGPU_MAX_LEVELS];        // strips per row of strips
    int nlevels;
};
static_assert(sizeof(StripGeom) == 4 * (2 * ORBGPU_MAX_LEVELS + 2), "StripGeom is a kernel argument");

struct DetectGeom {
    int first[ORBGPU_MAX_LEVELS + 1];  // first flat column strip of each level (bands x dword columns)
    int nsx[ORBGPU_MAX_LEVELS];        // dword columns per band: padded dwords 9 .. (w-1)/4
    int ncols[ORBGPU_MAX_LEVELS];      // cell columns of the level's cell grid (skipped ones excluded)
    int ctab_off[ORBGPU_MAX_LEVELS];   // first ColumnInfo of the level
    int xfirst[ORBGPU_MAX_LEVELS];     // image column of pixel 0 of the level's first strip: 17 for a padded plane (its aligned
                                       // dword 9), 16 for level 0 read directly from the image (Src0: aligned to the image)
    int nlevels;
};
static_assert(sizeof(DetectGeom) == 4 * (5 * ORBGPU_MAX_LEVELS + 2), "DetectGeom is a kernel argument");

struct ColumnInfo {
    uint32_t cellj;  // byte p: cell column of pixel p of the dword (0xFF: outside every cell interior)
    uint32_t flags;  // bit p: pixel p lies in a cell interior; bit 4+p: first column of its cell; bit 8+p: last column
};
static_assert(sizeof(ColumnInfo) == 8, "ColumnInfo is read as one 8-byte word");

struct UMax {
    int v[16];
};
static_assert(sizeof(UMax) == 64, "UMax: one entry per |v| <= HALF_PATCH");

ORBGPU_PLAN_HD int reflect101(int p, int len)
{
    // single bounce is enough: every level is >= 62 px and the border is 19 px
    if (p < 0)
        p = -p;
    else if (p >= len)
        p = 2 * (len - 1) - p;
    return p;
}

// a refusal: the message goes to *why, the status to the caller
#if defined(__GNUC__)
__attribute__((format(printf, 2, 3)))
#endif
inline int plan_refuse(std::string *why, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (why)
        *why = buf;
    return ORBGPU_EINVAL;
}
#define ORBGPU_PLAN_REQUIRE(cond, ...)              \
    do {                                            \
        if (!(cond))                                \
            return plan_refuse(why, __VA_ARGS__);   \
    } while (0)

// ---------------------------------------------------------------------------------------------
// E0: constructor tables, ORBextractor.cc:410-470
// ---------------------------------------------------------------------------------------------
struct ExtractorConsts {
    int nlevels = 0, nfeatures = 0;
    double scale_factor_d = 0;  // ORBextractor.h:98 keeps a double
    float scale[ORBGPU_MAX_LEVELS] = {}, inv_scale[ORBGPU_MAX_LEVELS] = {}, sigma2[ORBGPU_MAX_LEVELS] = {},
          inv_sigma2[ORBGPU_MAX_LEVELS] = {};
    int quota[ORBGPU_MAX_LEVELS] = {};
    UMax umax = {};
};

inline int build_consts(int nfeatures, float scale_factor, int nlevels, ExtractorConsts *c, std::string *why)
{
    ORBGPU_PLAN_REQUIRE(nlevels >= 1 && nlevels <= ORBGPU_MAX_LEVELS, "nlevels must be in [1,%d]", ORBGPU_MAX_LEVELS);
    const int nl = c->nlevels = nlevels;
    c->nfeatures = nfeatures;
    c->scale_factor_d = (double)scale_factor;
    c->scale[0] = 1.0f;
    c->sigma2[0] = 1.0f;
    for (int i = 1; i < nl; i++) {
        c->scale[i] = (float)((double)c->scale[i - 1] * c->scale_factor_d);
        c->sigma2[i] = c->scale[i] * c->scale[i];
    }
    for (int i = 0; i < nl; i++) {
        c->inv_scale[i] = 1.0f / c->scale[i];
        c->inv_sigma2[i] = 1.0f / c->sigma2[i];
    }
    const float factor = (float)(1.0 / c->scale_factor_d);
    float desired = (float)nfeatures * (1 - factor) / (1 - (float)pow((double)factor, (double)nl));
    int sum = 0;
    for (int l = 0; l < nl - 1; l++) {
        c->quota[l] = cv_round_host(desired);
        sum += c->quota[l];
        desired *= factor;
    }
    c->quota[nl - 1] = std::max(nfeatures - sum, 0);

    int *um = c->umax.v;
    const int vmax = (int)floor(HALF_PATCH * sqrtf(2.f) / 2 + 1);
    const int vmin = (int)ceil(HALF_PATCH * sqrtf(2.f) / 2);
    const double hp2 = HALF_PATCH * HALF_PATCH;
    for (int v = 0; v <= vmax; ++v)
        um[v] = cv_round_host(sqrt(hp2 - v * v));
    for (int v = HALF_PATCH, v0 = 0; v >= vmin; --v) {
        while (um[v0] == um[v0 + 1])
            ++v0;
        um[v] = v0;
        ++v0;
    }
    // k_orient's "third piece" rule is written for these values (half widths 15 up to |v| = 3, >= 14 up to |v| = 6)
    static const int expect[16] = {15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3};
    for (int v = 0; v <= HALF_PATCH; v++)
        ORBGPU_PLAN_REQUIRE(um[v] == expect[v], "umax[%d] = %d, k_orient is written for %d", v, um[v], expect[v]);
    return ORBGPU_OK;
}

// Size of pyramid level l of a w x h image (:1112) and the rectangle its FAST cells and quadtree nodes cover
// (maxBorder - minBorder, ORBextractor.cc:775-778)
struct LevelSize {
    int w, h;
    float width, height;
};
inline LevelSize level_size(const ExtractorConsts &c, int w, int h, int l)
{
    LevelSize s;
    s.w = cv_round_host((float)w * c.inv_scale[l]);
    s.h = cv_round_host((float)h * c.inv_scale[l]);
    s.width = (float)(s.w - 2 * BORDER0);
    s.height = (float)(s.h - 2 * BORDER0);
    return s;
}
// DistributeOctTree initial nodes, :542-544 (height > 0)
inline int level_n_ini(const LevelSize &s) { return (int)roundf(s.width / s.height); }
// E3': a level yields at most max(4*nIni, quota+2) key points
inline int level_max_keypoints(int n_ini, int quota) { return std::max(4 * n_ini, quota + 3); }

// REFLECT_101 frame of `ring` pixels around the interiors of levels >= 1 (k_ring_fill): items per level
inline RingGeom ring_geom(const std::vector<LevelGeom> &geom, int ring)
{
    RingGeom rg = {};
    rg.nlevels = (int)geom.size();
    for (int l = 1; l < rg.nlevels; l++)
        rg.first[l + 1] = rg.first[l] + 2 * ring * (geom[l].w + 2 * ring) + 2 * ring * geom[l].h;
    return rg;
}

static const int8_t k_pattern_host[1024] = {
#include "orbgpu_pattern.inc"
};

// ---------------------------------------------------------------------------------------------
// Everything one image size derives from the constructor tables
// ---------------------------------------------------------------------------------------------
struct PlanHooks {
    int qt_keys = -1;              // ORBGPU_DEBUG_QT_KEYS: LDS key share of k_quadtree<true>; -1 = as many as fit
    bool qt_no_prefilter = false;  // ORBGPU_DEBUG_QT_NOPRE
};

struct PlanTable {  // one constant table inside ExtractorPlan::blob
    size_t off = 0, bytes = 0;
};
constexpr size_t PLAN_ALIGN = 256;  // every table starts at a multiple of this

struct ExtractorPlan {
    int w = 0, h = 0;  // 0: nothing planned
    std::vector<LevelGeom> geom;
    int ncells = 0;
    StripGeom blur_geom = {};
    DetectGeom det_geom = {}, det_geom_direct = {};  // ... with level 0 aligned to the image (direct mode)
    RingGeom ring_full = {};                         // k_ring_fill with ring = EDGE: a whole padded plane is handed out
    size_t frame_pyr = 0, frame_slots = 0;           // bytes of planes / key slots per frame
    int sel_cap_total = 0, ncap = 0, max_kp = 0;
    size_t qt_lds = 0;
    int qt_kcap = 0;  // keys of a level k_quadtree<true> keeps in LDS
    int max_slots_level = 0;
    bool qt_prefilter = false;  // every level has <= QT_INI_MAX initial nodes
    bool border_fast = false;   // level-0 column table present (width % 4 == 0)
    // direct mode (Src0): level 0 read from the caller's image, no padded copy
    bool direct0_ok = false;  // the geometry has the tables for it (width % 8 == 0, >= 2 levels on the fast resize path)
    int rs_off_direct = 0;    // level 1's strip tables for the unpadded source
    int r8_off[ORBGPU_MAX_LEVELS] = {};  // 8-pixel form of k_resize_fast: first item of the level, -1 = the level keeps the 4-pixel form
    int r8_off_direct = -1;              // ... of level 1 for the unpadded source
    bool r8_share[ORBGPU_MAX_LEVELS] = {}, r8_share_direct = false;  // some item of the level has R8_SHARE set
    bool interior_resize = false;  // some level >= 1 goes through k_resize_fast (plane interiors + 3 px of border only)
    // the constant tables as the device holds them: one blob, every table at a PLAN_ALIGN-ed offset (an empty table has
    // an offset and no bytes)
    std::vector<uint8_t> blob;
    PlanTable t_geom, t_cells, t_ctab, t_bcol, t_xtab, t_ytab, t_yrow, t_rstrip, t_rsel, t_rwt, t_r8item, t_r8sel, t_r8wt,
        t_pattern, t_orient, t_slot_level;  // t_pattern: rBRIEF pattern; t_orient: k_orient's byte-weight tables;
                                            // t_slot_level: slot_level() of every selection slot, one byte each
    template <typename T> const T *table(const PlanTable &t) const { return reinterpret_cast<const T *>(blob.data() + t.off); }
    template <typename T> size_t count(const PlanTable &t) const { return t.bytes / sizeof(T); }
};

template <typename T> inline PlanTable plan_add_table(std::vector<uint8_t> &blob, const T *data, size_t n)
{
    PlanTable t;
    t.off = (blob.size() + PLAN_ALIGN - 1) / PLAN_ALIGN * PLAN_ALIGN;
    t.bytes = n * sizeof(T);
    blob.resize(t.off + t.bytes, 0);
    if (t.bytes)
        memcpy(blob.data() + t.off, data, t.bytes);
    return t;
}

// The level whose selection range [sel_off, sel_off + sel_cap) holds `slot`: the ranges are contiguous and ascending from 0
// (plan_extractor), so it is the number of levels >= 1 that start at or below the slot.  -1 for a slot outside every range.
inline int slot_level(const std::vector<LevelGeom> &geom, int slot)
{
    if (slot < 0 || geom.empty() || slot >= geom.back().sel_off + geom.back().sel_cap)
        return -1;
    int level = 0;
    for (size_t l = 1; l < geom.size(); l++)
        level += slot >= geom[l].sel_off ? 1 : 0;
    return level;
}

// k_fast_detect: bands (rows of cells) x dword columns, and what every dword column knows about the cell grid.  Every
// level a padded plane (strips = its aligned dwords from dword 9: image column 17), or -- direct0 -- level 0 read from the
// image itself (strips aligned to the image, from column 16).  False: some wave's cells are not FD_CELLS consecutive ids.
inline bool plan_detect(const std::vector<LevelGeom> &geom, bool direct0, DetectGeom &dgm, std::vector<ColumnInfo> &ctab)
{
    const int nl = (int)geom.size();
    memset(&dgm, 0, sizeof(dgm));
    dgm.nlevels = nl;
    int acc = 0;
    for (int l = 0; l < nl; l++) {
        const LevelGeom &g = geom[l];
        const bool dir = direct0 && l == 0;
        const int xfirst = dir ? 16 : 9 * 4 - EDGE;
        // strips must reach the last scored column, w - 20 (padded planes: up to their aligned dword (w-1)/4)
        const int nsx = dir ? (g.w - 20 - xfirst) / 4 + 1 : (g.w - 1) / 4 - 9 + 1;
        const int nbands = (g.h - 2 * EDGE + g.hcell - 1) / g.hcell;
        dgm.first[l] = acc;
        dgm.nsx[l] = nsx;
        dgm.ncols[l] = g.ncols_eff;
        dgm.ctab_off[l] = (int)ctab.size();
        dgm.xfirst[l] = xfirst;
        acc += nsx * nbands;
        if (dir)  // level 0's strips end on a wave boundary: a wave of k_fast_detect then reads ONE plane (image or pyramid)
            acc = (acc + FD_OWN - 1) / FD_OWN * FD_OWN;
        for (int sx = 0; sx < nsx; sx++) {
            ColumnInfo c{0u, 0u};
            for (int p = 0; p < 4; p++) {
                const int x = xfirst + 4 * sx + p;  // image column
                int j = 0xFF;
                if (x >= EDGE && x < g.w - EDGE) {
                    j = (x - EDGE) / g.wcell;
                    const int xs = EDGE + j * g.wcell, xe = std::min(xs + g.wcell, g.w - EDGE);  // interior [xs, xe)
                    if (j < g.ncols_eff) {
                        c.flags |= 1u << p;
                        if (x == xs)
                            c.flags |= 16u << p;
                        if (x == xe - 1)
                            c.flags |= 256u << p;
                    } else
                        j = 0xFF;
                }
                c.cellj |= (uint32_t)j << (8 * p);
            }
            ctab.push_back(c);
        }
    }
    for (int l = nl; l <= ORBGPU_MAX_LEVELS; l++)
        dgm.first[l] = acc;
    // the key emission of k_fast_detect addresses per-wave counters with (cell id mod FD_CELLS): the cells of the
    // columns a wave owns must be a range of at most FD_CELLS consecutive ids
    std::vector<std::pair<int, int>> strip_cells;  // per flat strip: lowest / highest cell id (-1: none)
    for (int l = 0; l < nl; l++) {
        const LevelGeom &g = geom[l];
        const int nbands = (g.h - 2 * EDGE + g.hcell - 1) / g.hcell;
        strip_cells.resize((size_t)dgm.first[l], {-1, -1});  // (the padding strips in front of this level)
        for (int b = 0; b < nbands; b++)
            for (int sx = 0; sx < dgm.nsx[l]; sx++) {
                const ColumnInfo &c = ctab[dgm.ctab_off[l] + sx];
                int lo = -1, hi = -1;
                for (int p = 0; p < 4; p++)
                    if ((c.flags >> p) & 1u) {
                        const int id = g.cell_first + b * dgm.ncols[l] + (int)((c.cellj >> (8 * p)) & 255u);
                        lo = lo < 0 ? id : std::min(lo, id);
                        hi = std::max(hi, id);
                    }
                strip_cells.push_back({lo, hi});
            }
    }
    for (size_t w0 = 0; w0 < strip_cells.size(); w0 += FD_OWN) {
        int lo = -1, hi = -1;
        for (size_t q = w0; q < std::min(w0 + FD_OWN, strip_cells.size()); q++)
            if (strip_cells[q].first >= 0) {
                lo = lo < 0 ? strip_cells[q].first : std::min(lo, strip_cells[q].first);
                hi = std::max(hi, strip_cells[q].second);
            }
        if (hi - lo >= FD_CELLS)
            return false;
    }
    return true;
}

// Level sizes, FAST cell grid, resize tables, slot layout for one image size.  ORBGPU_OK, or ORBGPU_EINVAL with the
// reason in *why (and *out unspecified).
inline int plan_extractor(const ExtractorConsts &cst, int w, int h, const PlanHooks &hooks, ExtractorPlan *out,
                          std::string *why)
{
    ExtractorPlan &P = *out;
    P = ExtractorPlan();
    const int nl = cst.nlevels;
    std::vector<LevelGeom> &geom = P.geom;
    geom.resize(nl);
    std::vector<CellDesc> cells;
    ResizeTables rt;
    std::vector<ResizeLevel> rlev(nl);
    size_t plane_off = 0;
    int slot_off = 0, sel_off = 0, max_cells_level = 0, ncap = 0;
    for (int l = 0; l < nl; l++) {
        LevelGeom &g = geom[l];
        memset(&g, 0, sizeof(g));
        const LevelSize ls = level_size(cst, w, h, l);
        g.w = ls.w;
        g.h = ls.h;
        g.max_bx = g.w - EDGE + 3;
        g.max_by = g.h - EDGE + 3;
        const float width = ls.width, height = ls.height;
        g.ncols = (int)(width / CELL_W);
        g.nrows = (int)(height / CELL_W);
        ORBGPU_PLAN_REQUIRE(g.ncols >= 1 && g.nrows >= 1 && g.w < 4096 + BORDER0 && g.h < 4096 + BORDER0,
                            "image %dx%d: pyramid level %d (%dx%d) is outside the supported range "
                            "(each level needs >= 62 px per side and < 4112 px)",
                            w, h, l, g.w, g.h);
        g.wcell = (int)ceilf(width / g.ncols);
        g.hcell = (int)ceilf(height / g.nrows);
        ORBGPU_PLAN_REQUIRE(g.wcell <= MAX_CELL && g.hcell <= MAX_CELL, "FAST cell %dx%d too large", g.wcell, g.hcell);
        g.pitch = ((g.w + 2 * EDGE + 63) / 64) * 64;
        g.plane_off = (int)plane_off;
        plane_off += (((size_t)g.pitch * (g.h + 2 * EDGE) + 255) / 256) * 256;
        g.quota = cst.quota[l];
        g.scale = cst.scale[l];
        g.patch = (int)(PATCH * cst.scale[l]);  // :837
        g.n_ini = level_n_ini(ls);
        ORBGPU_PLAN_REQUIRE(g.n_ini >= 1, "level %d aspect ratio unsupported (nIni = 0 divides by zero in the reference)", l);
        g.hx = width / (float)g.n_ini;
        // cells, :789-808
        g.cell_first = (int)cells.size();
        g.slot_off = slot_off;
        for (int i = 0; i < g.nrows; i++) {
            const float iniY = (float)(BORDER0 + i * g.hcell);
            float maxY = iniY + g.hcell + 6;
            if (iniY >= g.max_by - 3)
                continue;
            if (maxY > g.max_by)
                maxY = (float)g.max_by;
            for (int j = 0; j < g.ncols; j++) {
                const float iniX = (float)(BORDER0 + j * g.wcell);
                float maxX = iniX + g.wcell + 6;
                if (iniX >= g.max_bx - 6)
                    continue;
                if (maxX > g.max_bx)
                    maxX = (float)g.max_bx;
                CellDesc c;
                c.level = (short)l;
                c.x0 = (short)iniX;
                c.x1 = (short)maxX;
                c.y0 = (short)iniY;
                c.y1 = (short)maxY;
                c.addx = (short)(j * g.wcell);
                c.addy = (short)(i * g.hcell);
                const int iw = std::max(c.x1 - c.x0 - 6, 0), ih = std::max(c.y1 - c.y0 - 6, 0);
                // strict 3x3 NMS: no two survivors are 8-neighbours
                c.cap = (short)(((iw + 1) / 2) * ((ih + 1) / 2));
                c.slot_off = slot_off;
                c.pitch = g.pitch;
                c.plane_off = g.plane_off;
                c.pad[0] = 0;
                slot_off += c.cap;
                cells.push_back(c);
            }
        }
        g.ncells = (int)cells.size() - g.cell_first;
        g.slot_cnt = slot_off - g.slot_off;
        max_cells_level = std::max(max_cells_level, g.ncells);
        g.sel_cap = level_max_keypoints(g.n_ini, g.quota) + 1;
        g.sel_off = sel_off;
        sel_off += g.sel_cap;
        ncap = std::max(ncap, g.sel_cap);
        // resize tables (cv::resize INTER_LINEAR 8U, A2) and the item tables of k_resize_fast: resize_tables.h
        if (l > 0) {
            rlev[l] = resize_add_level(rt, geom[l - 1].w, geom[l - 1].h, geom[l - 1].pitch, g.w, g.h, g.pitch);
            g.xtab_off = rlev[l].xtab_off;
            g.ytab_off = rlev[l].ytab_off;
            g.yrow_off = rlev[l].yrow_off;
            g.rs_off = rlev[l].rs_off;
            g.rs_fast = rlev[l].fast4 ? 1 : 0;
        }
    }
    // direct mode: level 1's items once more, for source columns counted from the image's own column 0 (Src0)
    bool direct_ok = nl >= 2 && w % 8 == 0 && w >= 64 && geom[std::min(1, nl - 1)].rs_fast != 0;
    ResizeLevel rdirect;
    if (direct_ok) {
        rdirect = resize_add_direct(rt, rlev[1], geom[0].w, geom[1].w, geom[1].pitch);
        direct_ok = rdirect.fast4;
    }
    ncap = std::max(ncap, (max_cells_level + 3) / 4);  // the cell scan reuses the [ncap*4] child-count array
    ncap = ((ncap + 7) / 8) * 8;
    // k_quadtree's dynamic LDS per node slot: two short4 boxes, two ints, eight ints, two ints, 2 x four u16, a byte, two u32
    const size_t qt_lds = (size_t)ncap * (2 * sizeof(short[4]) + 2 * sizeof(int) + 8 * sizeof(int) + 2 * sizeof(int) +
                                          4 * sizeof(uint16_t) + 4 * sizeof(uint16_t) + 1 + 2 * sizeof(uint32_t)) + 64;
    // single frames: keys (4 B) and node ids (2 B) of a level in LDS, as many as fit (never more than a level can hold)
    int max_slots_level = 0;
    for (int l = 0; l < nl; l++)
        max_slots_level = std::max(max_slots_level, geom[l].slot_cnt);
    int qt_kcap = max_slots_level;
    if (hooks.qt_keys >= 0)  // test hook: forces the mixed LDS / memory path
        qt_kcap = hooks.qt_keys;
    qt_kcap = (int)std::min<size_t>((size_t)(qt_kcap + 7) / 8 * 8, qt_lds < 150 * 1024 ? (150 * 1024 - qt_lds) / 6 / 8 * 8 : 0);
    ORBGPU_PLAN_REQUIRE(qt_lds <= (size_t)QT_LDS_MAX, "nfeatures too large for the quadtree kernel (needs %zu B of LDS)", qt_lds);
    ORBGPU_PLAN_REQUIRE((size_t)slot_off < (1u << 23), "too many FAST key slots per frame");

    {
        StripGeom &bgm = P.blur_geom;
        bgm.nlevels = nl;
        int acc = 0;
        for (int l = 0; l < nl; l++) {
            // 8-pixel strips (two dwords) start at padded dword 4 (bytes 16..19 hold image column 0) and must cover
            // column w-1
            const int nsx = ((geom[l].w + EDGE - 1) / 4 - 4 + 1 + 1) / 2;
            const int nsy = (geom[l].h + BLUR_ROWS - 1) / BLUR_ROWS;
            bgm.first[l] = acc;
            bgm.nsx[l] = nsx;
            acc += nsx * nsy;
        }
        for (int l = nl; l <= ORBGPU_MAX_LEVELS; l++)
            bgm.first[l] = acc;
    }
    for (int l = 0; l < nl; l++) {
        LevelGeom &g = geom[l];
        int ncols_eff = 0;  // cell columns that are not skipped (ORBextractor.cc:797: iniX >= maxBorderX-6)
        for (int j = 0; j < g.ncols; j++)
            if (BORDER0 + j * g.wcell < g.max_bx - 6)
                ncols_eff++;
        const int nbands = (g.h - 2 * EDGE + g.hcell - 1) / g.hcell;  // bands with interior rows
        ORBGPU_PLAN_REQUIRE(ncols_eff > 0 && g.ncells % ncols_eff == 0 && nbands <= g.ncells / ncols_eff && ncols_eff < 255 &&
                                g.ncells / ncols_eff < 256 && g.hcell < 128,
                            "unexpected cell grid at level %d", l);
        g.ncols_eff = ncols_eff;
        for (int which = 0; which < 2; which++) {
            const int d = which ? g.hcell : g.wcell;
            const uint32_t m = (uint32_t)(((1ull << 32) + (uint64_t)d - 1u) / (uint64_t)d);
            for (uint32_t v = 0; v < 8192u; v++)
                ORBGPU_PLAN_REQUIRE((uint32_t)(((uint64_t)v * m) >> 32) == v / (uint32_t)d, "cell size %d at level %d has no exact reciprocal", d, l);
            (which ? g.inv_hcell : g.inv_wcell) = m;
        }
    }
    std::vector<ColumnInfo> ctab;
    ORBGPU_PLAN_REQUIRE(plan_detect(geom, false, P.det_geom, ctab),
                        "image too small for the FAST kernel's cell bookkeeping (more than %d cells in one wave)", FD_CELLS);
    if (direct_ok)
        direct_ok = plan_detect(geom, true, P.det_geom_direct, ctab);
    P.direct0_ok = direct_ok;
    P.rs_off_direct = rdirect.rs_off;
    for (int l = 0; l < ORBGPU_MAX_LEVELS; l++)
        P.r8_off[l] = l >= 1 && l < nl && rlev[l].fast8 ? rlev[l].r8_off : -1;
    P.r8_off_direct = direct_ok && rdirect.fast8 ? rdirect.r8_off : -1;
    for (int l = 0; l < ORBGPU_MAX_LEVELS; l++)
        P.r8_share[l] = l >= 1 && l < nl && rlev[l].share8;
    P.r8_share_direct = rdirect.share8;
    for (int l = 1; l < nl; l++)
        P.interior_resize = P.interior_resize || geom[l].rs_fast != 0;
    P.ring_full = ring_geom(geom, EDGE);
    // k_border0_fast: per aligned dword of the padded level-0 row, the two adjacent source dwords and the byte selector
    std::vector<BorderCol> bcol;
    if (w % 4 == 0 && w >= 8) {
        const LevelGeom &g0 = geom[0];
        for (int c = 0; c < g0.pitch / 4; c++) {
            int sx[4], lo = 1 << 30, hi = 0;
            for (int k = 0; k < 4; k++) {
                sx[k] = reflect101(std::min(c * 4 + k, g0.w + 2 * EDGE - 1) - EDGE, g0.w);
                lo = std::min(lo, sx[k]);
                hi = std::max(hi, sx[k]);
            }
            const int d = std::min(lo / 4, g0.w / 4 - 2);  // src[d + 1] stays inside the row
            ORBGPU_PLAN_REQUIRE(hi < d * 4 + 8 && lo >= d * 4, "level-0 border table: span of column %d", c);
            BorderCol bc{(uint32_t)d, 0u};
            for (int k = 0; k < 4; k++)
                bc.sel |= (uint32_t)(sx[k] - d * 4) << (8 * k);  // bytes 0..3 = src[d], 4..7 = src[d+1]
            bcol.push_back(bc);
        }
    }
    P.border_fast = !bcol.empty();
    // k_orient's byte-weight tables per (alignment a of the disc's first column, |v|, dword j of the 9-dword row):
    // W10 holds u + 16 inside the disc (0 outside), M01 holds 1 inside the disc
    std::vector<uint32_t> orw(2 * 4 * 16 * 9, 0u);
    for (int i = 0; i < 4 * 16 * 9; i++) {
        const int a = i / (16 * 9), av = (i / 9) % 16, j = i % 9;
        for (int k = 0; k < 4; k++) {
            const int u = 4 * j + k - a - HALF_PATCH;
            if (std::abs(u) <= cst.umax.v[av]) {
                orw[i] |= (uint32_t)(u + 16) << (8 * k);
                orw[4 * 16 * 9 + i] |= 1u << (8 * k);
            }
        }
    }
    P.w = w;
    P.h = h;
    P.ncells = (int)cells.size();
    P.frame_pyr = plane_off;
    P.frame_slots = (size_t)slot_off;
    P.sel_cap_total = sel_off;
    P.ncap = ncap;
    P.qt_lds = qt_lds;
    P.qt_kcap = qt_kcap;
    P.max_slots_level = max_slots_level;
    P.qt_prefilter = !hooks.qt_no_prefilter;
    for (int l = 0; l < nl; l++) {
        P.qt_prefilter = P.qt_prefilter && geom[l].n_ini <= QT_INI_MAX;
        P.max_kp += geom[l].sel_cap - 1;
    }
    std::vector<uint8_t> &b = P.blob;
    P.t_geom = plan_add_table(b, geom.data(), geom.size());
    P.t_cells = plan_add_table(b, cells.data(), cells.size());
    P.t_ctab = plan_add_table(b, ctab.data(), ctab.size());
    P.t_bcol = plan_add_table(b, bcol.data(), bcol.size());
    P.t_xtab = plan_add_table(b, rt.xtab.data(), rt.xtab.size());
    P.t_ytab = plan_add_table(b, rt.ytab.data(), rt.ytab.size());
    P.t_yrow = plan_add_table(b, rt.yrow.data(), rt.yrow.size());
    P.t_rstrip = plan_add_table(b, rt.strip.data(), rt.strip.size());
    P.t_rsel = plan_add_table(b, rt.sel.data(), rt.sel.size());
    P.t_rwt = plan_add_table(b, rt.wt.data(), rt.wt.size());
    P.t_r8item = plan_add_table(b, rt.item8.data(), rt.item8.size());
    P.t_r8sel = plan_add_table(b, rt.sel8.data(), rt.sel8.size());
    P.t_r8wt = plan_add_table(b, rt.wt8.data(), rt.wt8.size());
    P.t_pattern = plan_add_table(b, k_pattern_host, sizeof(k_pattern_host));
    P.t_orient = plan_add_table(b, orw.data(), orw.size());
    // k_orient: the level of every selection slot of a frame (a kernel finds its level with one byte load)
    std::vector<uint8_t> slot_lev((size_t)sel_off);
    for (int s = 0; s < sel_off; s++)
        slot_lev[(size_t)s] = (uint8_t)slot_level(geom, s);
    P.t_slot_level = plan_add_table(b, slot_lev.data(), slot_lev.size());
    return ORBGPU_OK;
}

// ---------------------------------------------------------------------------------------------
// Launch decisions that depend on the batch of a call
// ---------------------------------------------------------------------------------------------
// k_quadtree: the batch variant keeps no keys in LDS; single frames keep the plan's share and get more threads
struct QuadtreeLaunch {
    bool lds_keys;  // k_quadtree<true>
    int kcap, threads;
    size_t lds_bytes;
};
inline QuadtreeLaunch quadtree_launch(const ExtractorPlan &p, int batch, bool force_batch_variant)
{
    if (batch >= QT_BATCH_MIN || force_batch_variant)
        return QuadtreeLaunch{false, 0, QT_THREADS_BATCH, p.qt_lds};
    return QuadtreeLaunch{true, p.qt_kcap, p.w * p.h >= QT_LARGE_PIXELS ? QT_THREADS : QT_THREADS_SMALL,
                          p.qt_lds + (size_t)p.qt_kcap * 6};
}

// The form level l >= 1 is resized in.  direct: the call reads level 0 from the caller's image.
struct ResizeLaunch {
    int px;      // 0: k_resize_level (the general kernel); 4 / 8: pixels per item of k_resize_fast
    int rows;    // padded rows per item (k_resize_fast)
    bool share;  // 8-pixel form: some item of the level has R8_SHARE set
    bool dir1;   // level 1 straight from the image
    int off;     // first strip (4-pixel form) / first item (8-pixel form) of the level's tables
};
inline ResizeLaunch resize_launch(const ExtractorPlan &p, int l, int batch, bool direct)
{
    const LevelGeom &g = p.geom[l];
    if (!g.rs_fast)
        return ResizeLaunch{0, 0, false, false, 0};
    const bool dir1 = direct && l == 1;
    // a batch: eight pixels per item where the level's taps fit the 16-byte window (resize_tables.h)
    const int r8 = batch >= PYR_BATCH_MIN ? (dir1 ? p.r8_off_direct : p.r8_off[l]) : -1;
    if (r8 >= 0)
        return ResizeLaunch{8, PYR_ROWS, dir1 ? p.r8_share_direct : p.r8_share[l], dir1, r8};
    // rows per thread: 8 on the large levels; the small ones of a few frames get more (shorter) threads to hide
    // latency with.  A batch has threads enough: every level takes full items and keeps its horizontal passes.
    const int ndw_l = (g.pitch / 4) * (g.h + 2 * EDGE);
    const int rows = batch >= PYR_BATCH_MIN || ndw_l >= 32768 ? PYR_ROWS : ndw_l >= 16384 ? PYR_ROWS / 2 : PYR_ROWS / 4;
    return ResizeLaunch{4, rows, false, dir1, dir1 ? p.rs_off_direct : g.rs_off};
}

}  // namespace orbgpu
