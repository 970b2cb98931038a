// Host side of the pyramid resize chain (k_resize_fast / k_resize_level, extractor.hip): cv::resize's INTER_LINEAR 8-bit
// tables of a level (OpenCV 2.4 fixed point), the per-item window, selector and weight tables of the two
// forms of k_resize_fast, and the decision whether a level may take them.  Host-only, no HIP: compiles with plain
// g++ -std=c++17 (tests/resize_tables_test.cpp), so the windows can be checked without a device.
//
// k_resize_fast writes the interior of a padded plane and RS_RING pixels of REFLECT_101 border around it (what the 7x7
// blur reads; no other stage reads the border): rows 0 .. h-1 -- rows 1 .. RS_RING and h-1-RS_RING .. h-2 are
// stored a second time as the border rows they reflect to -- and the aligned dword columns RESIZE_DW0 .. RESIZE_DW0 +
// resize_ndw(w) - 1 that hold the columns -RS_RING .. w-1+RS_RING.  A border slot takes the taps of the column it reflects
// to (only the first and the last dwords of a row hold any; their taps are the only ones that ever decrease from slot to
// slot); slots further out take those of the outermost ring column and produce bytes nobody reads.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

namespace orbgpu {

constexpr int RS_EDGE = 19;                 // EDGE_THRESHOLD: border of a padded plane (extractor.hip asserts it is its EDGE)
constexpr int RS_RING = 3;                  // border pixels the resize chain writes itself
constexpr int RESIZE_DW0 = (RS_EDGE - RS_RING) >> 2;  // first aligned dword column of a padded row that k_resize_fast writes
constexpr int resize_ndw(int w) { return ((RS_EDGE + w - 1 + RS_RING) >> 2) - RESIZE_DW0 + 1; }  // how many of them
constexpr int resize_n8(int w) { return (resize_ndw(w) + 1) >> 1; }                    // 8-pixel items per row

struct XTab {  // cv::resize horizontal table entry (A2)
    uint16_t sx, sx1, a0, a1;
};
struct YTab {
    uint16_t sy0, sy1;
    int16_t b0, b1;
};
struct YRow {  // the same per PADDED output row (border rows = the entry of the row they reflect to), as four ints: one
    int sy0, sy1, b0, b1;  // 16-byte load, no reflection and no field extraction in k_resize_fast's row loop
};
struct ResizeStrip {  // 4-pixel form, per padded output dword column of a level (only those that hold an image column are used)
    uint32_t base_q;  // bits 0..15: window base (source column, multiple of 4); bits 16..17: byte shift of the window;
                      // bit 18 (direct level-0 source only): the window is the last 12 bytes of the row and the pair comes from its dwords 1, 2
};
struct RsQuad {  // four selectors or four (left | right << 16) weight pairs: read as one 16-byte word
    uint32_t x, y, z, w;
};
// 8-pixel form, one word per item (output padded columns 4 RESIZE_DW0 + 8 i .. + 7).  The item loads ONE 16-byte window
// per source row at byte `base` of the row and shifts it by `shift` bytes: run byte j = window byte 4 rot + shift + j.  Slots 0..3 (half 0) take their taps from run bytes 0..7, slots 4..7 (half 1) from
// run bytes 4 + e .. 11 + e (with R8_SHARE: from run bytes 0..7 as well).  Every tap of every slot lies inside the window.
// R8_SHARE costs the kernel two selects per source row: a level none of whose items needs it runs without (share8).
constexpr uint32_t R8_BASE_MASK = 0xFFFFu;  // bits 0..15: window base (source column, multiple of 4)
constexpr int R8_SHIFT_LSB = 16;            // bits 16..17: shift
constexpr int R8_ROT_LSB = 18;              // bits 18..19, direct source only: rot = 1, 2: the window is the row's last 16 bytes, the run starts in its dword rot
constexpr int R8_E_LSB = 20;                // bits 20..21: e
constexpr uint32_t R8_SHARE = 1u << 22;     // half 1 shares half 0's eight bytes (the first item of a row, whose first slots reflect)

inline int cv_round_host(double v) { return (int)lrint(v); }
inline short sat_short(int v) { return (short)(v < -32768 ? -32768 : v > 32767 ? 32767 : v); }
inline int rs_reflect101(int p, int len) { return p < 0 ? -p : p >= len ? 2 * (len - 1) - p : p; }
// v_perm_b32 selector of one slot: (left tap, zero, right tap, zero) out of eight bytes
inline uint32_t rs_selector(int ol, int orr) { return (uint32_t)(ol & 7) | 0x0c00u | ((uint32_t)(orr & 7) << 16) | 0x0c000000u; }

struct ResizeTables {
    std::vector<XTab> xtab;  // per level: one entry per output column
    std::vector<YTab> ytab;  // per level: one entry per output row
    std::vector<YRow> yrow;  // per level: one entry per PADDED output row
    std::vector<ResizeStrip> strip;  // 4-pixel form: per level (and once more for the direct source) one entry per padded dword column
    std::vector<RsQuad> sel, wt;     // ... its four selectors and weight pairs
    std::vector<uint32_t> item8;     // 8-pixel form: per level (and the direct source) one word per item
    std::vector<RsQuad> sel8, wt8;   // ... its eight selectors and weight pairs (two quads per item)
};
struct ResizeLevel {
    int xtab_off = 0, ytab_off = 0, yrow_off = 0;
    int rs_off = 0, r8_off = 0;      // first ResizeStrip / first 8-pixel item of the level
    bool fast4 = false, fast8 = false;  // the level may take the 4-pixel / the 8-pixel form of k_resize_fast
    bool rows_pos = false;              // no row weight is negative (the 8-pixel form multiplies them as unsigned values)
    bool share8 = false;                // some item of the 8-pixel form has R8_SHARE set
};

// image column of slot k of the padded dword column sdw: itself, or the one a ring column reflects to
inline int rs_slot_column(int sdw, int k, int dw)
{
    return rs_reflect101(std::min(std::max(sdw * 4 + k - RS_EDGE, -RS_RING), dw - 1 + RS_RING), dw);
}

// 4-pixel form: the 12-byte window of every dword column, shifted so that all eight taps of its four slots lie in ONE
// 8-byte pair.  src_off: column of source pixel 0 in a source row (RS_EDGE for a padded plane).
inline bool resize_strips4(const XTab *xt, int dw, int dpitch, int src_off, ResizeTables &T)
{
    bool ok = true;
    for (int sdw = 0; sdw < dpitch / 4; sdw++) {
        int cl[4], cr[4], mn = 1 << 30;
        const XTab *x[4];
        for (int k = 0; k < 4; k++) {
            x[k] = &xt[rs_slot_column(sdw, k, dw)];
            cl[k] = x[k]->sx + src_off;
            cr[k] = x[k]->sx1 + src_off;
            mn = std::min(mn, cl[k]);
        }
        // the window starts at the aligned column wbase; the kernel shifts it by sh = mn - wbase bytes (two v_alignbyte
        // per source row)
        const int wbase = mn & ~3, sh = mn - wbase;
        uint32_t sel[4], wt[4];
        for (int k = 0; k < 4; k++) {
            const int ol = cl[k] - mn, orr = cr[k] - mn;
            if (ol < 0 || orr < ol || orr > 7)
                ok = false;
            sel[k] = rs_selector(ol, orr);
            wt[k] = (uint32_t)x[k]->a0 | ((uint32_t)x[k]->a1 << 16);
        }
        T.strip.push_back(ResizeStrip{(uint32_t)wbase | ((uint32_t)sh << 16)});
        T.sel.push_back(RsQuad{sel[0], sel[1], sel[2], sel[3]});
        T.wt.push_back(RsQuad{wt[0], wt[1], wt[2], wt[3]});
    }
    return ok;
}

// 4-pixel form for the direct source: level 1's strips once more, for source columns counted from the image's own column 0.
// A window that would run past the end of an image row (the next row, or -- last row of the last frame -- the end of the
// caller's buffer) is placed on the row's last 12 bytes and the pair is cut from its second and third dword (bit 18).
inline bool resize_strips4_direct(const XTab *xt, int dw, int dpitch, int sw, ResizeTables &T)
{
    bool ok = true;
    for (int sdw = 0; sdw < dpitch / 4; sdw++) {
        int cl[4], cr[4], mn = 1 << 30;
        const XTab *x[4];
        for (int k = 0; k < 4; k++) {
            x[k] = &xt[rs_slot_column(sdw, k, dw)];
            cl[k] = x[k]->sx;
            cr[k] = x[k]->sx1;
            mn = std::min(mn, cl[k]);
        }
        int wbase = mn & ~3, ps = mn;  // ps: first byte of the 8-byte pair the selectors index
        int pbase = wbase;             // first byte of the two dwords the pair is cut from
        uint32_t edge = 0;
        if (wbase + 12 > sw) {  // the window would pass the end of the row: the row's last 12 bytes, pair from dwords 1 and 2
            wbase = sw - 12;
            pbase = sw - 8;
            ps = std::min(mn, pbase + 3);
            edge = 1u << 18;
        }
        const int sh = ps - pbase;
        uint32_t sel[4], wt[4];
        for (int k = 0; k < 4; k++) {
            const int ol = cl[k] - ps, orr = cr[k] - ps;
            // inside the pair, and -- at a row end -- inside its valid part (the bytes above 7 - sh come from the re-read dword)
            if (sh < 0 || sh > 3 || wbase < 0 || ol < 0 || orr < ol || orr > (edge ? 7 - sh : 7))
                ok = false;
            sel[k] = rs_selector(ol, orr);
            wt[k] = (uint32_t)x[k]->a0 | ((uint32_t)x[k]->a1 << 16);
        }
        T.strip.push_back(ResizeStrip{(uint32_t)wbase | ((uint32_t)sh << 16) | edge});
        T.sel.push_back(RsQuad{sel[0], sel[1], sel[2], sel[3]});
        T.wt.push_back(RsQuad{wt[0], wt[1], wt[2], wt[3]});
    }
    return ok;
}

// 8-pixel form.  row_len: readable bytes of a source row (the pitch of a padded plane, the image width for the direct
// source: nothing outside an image row may be read).  The run starts at the largest byte R both halves and the window
// allow -- half 0 needs its first tap at or after R, half 1 at or after R + 4 -- and e moves half 1's eight bytes up to
// its first tap.
// Returns false, with the level's entries incomplete, as soon as a tap of some slot does not fit: the level then keeps
// the 4-pixel form.
inline bool resize_items8(const XTab *xt, int dw, int src_off, int row_len, bool direct, ResizeTables &T, bool *any_share)
{
    *any_share = false;
    for (int i = 0; i < resize_n8(dw); i++) {
        int cl[8], cr[8], mn0 = 1 << 30, mn1 = 1 << 30;
        const XTab *x[8];
        for (int k = 0; k < 8; k++) {
            x[k] = &xt[rs_slot_column(RESIZE_DW0 + 2 * i + (k >> 2), k & 3, dw)];
            cl[k] = x[k]->sx + src_off;
            cr[k] = x[k]->sx1 + src_off;
            (k < 4 ? mn0 : mn1) = std::min(k < 4 ? mn0 : mn1, cl[k]);
        }
        bool found = false;
        for (int variant = 0; variant < (direct ? 48 : 16) && !found; variant++) {
            // (the largest start first; a lower one only helps where the start is tied to the row's end)
            const bool share = (variant & 8) != 0;
            const int rot = direct ? variant >> 4 : 0;
            const int R = (share ? std::min(mn0, mn1) : std::min(mn0, mn1 - 4)) - (variant & 7);
            const int e = share ? 0 : std::min(mn1 - 4 - R, 3);
            const int wbase = rot ? row_len - 16 : R & ~3;
            const int sh = R - wbase - 4 * rot;
            if (R < 0 || wbase < 0 || (wbase & 3) != 0 || wbase + 16 > row_len || wbase > (int)R8_BASE_MASK || sh < 0 || sh > 3)
                continue;
            const int P[2] = {R, share ? R : R + 4 + e};
            bool fit = true;
            uint32_t sel[8], wt[8];
            for (int k = 0; k < 8; k++) {
                const int ol = cl[k] - P[k >> 2], orr = cr[k] - P[k >> 2];
                if (ol < 0 || orr < ol || orr > 7 || cr[k] >= wbase + 16)
                    fit = false;
                sel[k] = rs_selector(ol, orr);
                wt[k] = (uint32_t)x[k]->a0 | ((uint32_t)x[k]->a1 << 16);
            }
            if (!fit)
                continue;
            found = true;
            *any_share = *any_share || share;
            T.item8.push_back((uint32_t)wbase | ((uint32_t)sh << R8_SHIFT_LSB) | ((uint32_t)rot << R8_ROT_LSB) |
                              (share ? R8_SHARE : 0u) | ((uint32_t)e << R8_E_LSB));
            T.sel8.push_back(RsQuad{sel[0], sel[1], sel[2], sel[3]});
            T.sel8.push_back(RsQuad{sel[4], sel[5], sel[6], sel[7]});
            T.wt8.push_back(RsQuad{wt[0], wt[1], wt[2], wt[3]});
            T.wt8.push_back(RsQuad{wt[4], wt[5], wt[6], wt[7]});
        }
        if (!found)
            return false;
    }
    return true;
}

// The tables of one level (dw x dh, padded row pitch dpitch) resized from a level of sw x sh (padded row pitch spitch).
inline ResizeLevel resize_add_level(ResizeTables &T, int sw, int sh, int spitch, int dw, int dh, int dpitch)
{
    ResizeLevel L;
    L.xtab_off = (int)T.xtab.size();
    L.ytab_off = (int)T.ytab.size();
    const double scale_x = 1. / ((double)dw / sw), scale_y = 1. / ((double)dh / sh);
    for (int dx = 0; dx < dw; dx++) {
        float fx = (float)((dx + 0.5) * scale_x - 0.5);
        int sx = (int)floor(fx);
        fx -= sx;
        if (sx < 0) {
            fx = 0;
            sx = 0;
        }
        if (sx >= sw - 1) {
            fx = 0;
            sx = sw - 1;
        }
        XTab t;
        t.sx = (uint16_t)sx;
        t.sx1 = (uint16_t)std::min(sx + 1, sw - 1);
        t.a0 = (uint16_t)sat_short(cv_round_host((1.f - fx) * 2048));
        t.a1 = (uint16_t)sat_short(cv_round_host(fx * 2048));
        T.xtab.push_back(t);
    }
    bool pos = true;
    for (int dy = 0; dy < dh; dy++) {
        float fy = (float)((dy + 0.5) * scale_y - 0.5);
        int sy = (int)floor(fy);
        fy -= sy;
        YTab t;
        t.sy0 = (uint16_t)std::min(std::max(sy, 0), sh - 1);
        t.sy1 = (uint16_t)std::min(std::max(sy + 1, 0), sh - 1);
        t.b0 = sat_short(cv_round_host((1.f - fy) * 2048));
        t.b1 = sat_short(cv_round_host(fy * 2048));
        pos = pos && t.b0 >= 0 && t.b1 >= 0;
        T.ytab.push_back(t);
    }
    L.yrow_off = (int)T.yrow.size();
    for (int py = 0; py < dh + 2 * RS_EDGE; py++) {
        const YTab &t = T.ytab[L.ytab_off + rs_reflect101(py - RS_EDGE, dh)];
        T.yrow.push_back(YRow{(int)t.sy0, (int)t.sy1, (int)t.b0, (int)t.b1});
    }
    L.rs_off = (int)T.strip.size();
    L.fast4 = resize_strips4(&T.xtab[L.xtab_off], dw, dpitch, RS_EDGE, T);
    L.r8_off = (int)T.item8.size();
    L.rows_pos = pos;
    L.fast8 = L.fast4 && pos && resize_items8(&T.xtab[L.xtab_off], dw, RS_EDGE, spitch, false, T, &L.share8);
    if (!L.fast8) {  // (keep the arrays consistent: a refused level leaves no entries behind)
        T.item8.resize(L.r8_off);
        T.sel8.resize(2 * (size_t)L.r8_off);
        T.wt8.resize(2 * (size_t)L.r8_off);
    }
    return L;
}

// The same level once more with the caller's image (sw bytes per row, pixel 0 at byte 0) as its source: rs_off / r8_off
// and fast4 / fast8 of the direct source (the x, y and row tables are the level's own).
inline ResizeLevel resize_add_direct(ResizeTables &T, const ResizeLevel &lv, int sw, int dw, int dpitch)
{
    ResizeLevel L = lv;
    L.rs_off = (int)T.strip.size();
    L.fast4 = resize_strips4_direct(&T.xtab[lv.xtab_off], dw, dpitch, sw, T);
    L.r8_off = (int)T.item8.size();
    L.fast8 = L.fast4 && lv.rows_pos && sw >= 16 && sw % 4 == 0 && resize_items8(&T.xtab[lv.xtab_off], dw, 0, sw, true, T, &L.share8);
    if (!L.fast8) {
        T.item8.resize(L.r8_off);
        T.sel8.resize(2 * (size_t)L.r8_off);
        T.wt8.resize(2 * (size_t)L.r8_off);
    }
    return L;
}

}  // namespace orbgpu
