// CPU-side unit test of the resize chain's host tables (orb_slam2_map_amd/csrc/resize_tables.h): the windows, selectors
// and weights of both forms of k_resize_fast are checked slot by slot (image columns and the 3 ring columns on either
// side, which take the taps of the columns they reflect to), the two forms are run on the host with the
// kernel's own byte operations (v_alignbyte, v_perm, v_dot2 restated below) over planes whose borders hold 0xA5 and over
// an image buffer of exactly w x h bytes (the direct source: a window past a row's end would leave the allocation), and
// the result is compared with the plain integer formula of k_resize_level.
//
//   resize_tables_test W H SCALE MAXLEVELS IMAGE OUT
// reads W x H bytes from IMAGE, writes the interiors of levels 1 .. n-1 to OUT (the caller compares them with the
// oracle's pyramid) and prints "levels n fast8 <levels in the 8-pixel form> direct8 <0|1>".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "resize_tables.h"

using namespace orbgpu;

#define CHECK(c, ...)                                                                                                \
    do {                                                                                                             \
        if (!(c)) {                                                                                                  \
            printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #c);                                                     \
            printf(__VA_ARGS__);                                                                                     \
            printf("\n");                                                                                            \
            exit(1);                                                                                                 \
        }                                                                                                            \
    } while (0)

static uint32_t alignbyte(uint32_t hi, uint32_t lo, uint32_t sh)
{
    return (uint32_t)(((((uint64_t)hi << 32) | lo) >> (8 * (sh & 3))) & 0xFFFFFFFFu);
}
static uint32_t perm(uint32_t hi, uint32_t lo, uint32_t sel)
{
    const uint64_t v = ((uint64_t)hi << 32) | lo;
    uint32_t r = 0;
    for (int k = 0; k < 4; k++) {
        const uint32_t s = (sel >> (8 * k)) & 0xFF;
        CHECK(s < 8 || s == 0x0c, "selector byte %u", s);
        if (s < 8)
            r |= (uint32_t)((v >> (8 * s)) & 0xFF) << (8 * k);
    }
    return r;
}
static uint32_t dot2(uint32_t a, uint32_t b) { return (a & 0xFFFF) * (b & 0xFFFF) + (a >> 16) * (b >> 16); }
static uint32_t ld32(const uint8_t *p)
{
    uint32_t v;
    memcpy(&v, p, 4);
    return v;
}

struct Plane {  // a padded plane whose border holds 0xA5: the resize chain reads interiors only
    int w, h, pitch;
    std::vector<uint8_t> px;
    Plane(int w_, int h_) : w(w_), h(h_), pitch(((w_ + 2 * RS_EDGE + 63) / 64) * 64), px((size_t)pitch * (h_ + 2 * RS_EDGE), 0xA5) {}
    uint8_t *at(int x, int y) { return &px[(size_t)(y + RS_EDGE) * pitch + x + RS_EDGE]; }
    const uint8_t *row0(int y) const { return &px[(size_t)(y + RS_EDGE) * pitch]; }  // byte 0 of the padded row of image row y
};

// the image column a slot at column x (relative to the image) stands for: itself, the column a ring column reflects to
// (REFLECT_101), or -1 for a slot further out, whose output nobody reads
static int slot_column(int x, int w)
{
    if (x >= 0 && x < w)
        return x;
    if (x < 0 && x >= -RS_RING)
        return -x;
    if (x >= w && x < w + RS_RING)
        return 2 * (w - 1) - x;
    return -1;
}

static int vertical(int b0, int b1, int t0, int t1) { return ((((b0 * (t0 >> 4)) >> 16) + ((b1 * (t1 >> 4)) >> 16) + 2) >> 2) & 0xFF; }

// the 4-pixel form's horizontal pass of one padded dword column over one source row (row = byte 0 of the row)
static void h4(const uint8_t *row, uint32_t bq, const RsQuad &sel, const RsQuad &wt, bool direct, int t[4])
{
    const uint8_t *w = row + (bq & 0xFFFFu);
    uint32_t a0 = ld32(w), a1 = ld32(w + 4);
    const uint32_t a2 = ld32(w + 8), sh = (bq >> 16) & 3u;
    if (direct && ((bq >> 18) & 1u)) {
        a0 = a1;
        a1 = a2;
    }
    const uint32_t lo = alignbyte(a1, a0, sh), hi = alignbyte(a2, a1, sh);
    const uint32_t s[4] = {sel.x, sel.y, sel.z, sel.w}, wv[4] = {wt.x, wt.y, wt.z, wt.w};
    for (int k = 0; k < 4; k++)
        t[k] = (int)dot2(perm(hi, lo, s[k]), wv[k]);
}

// the 8-pixel form's
static void h8(const uint8_t *row, uint32_t bq, const RsQuad *sel, const RsQuad *wt, bool direct, int t[8])
{
    const uint8_t *w = row + (bq & R8_BASE_MASK);
    uint32_t d0 = ld32(w), d1 = ld32(w + 4), d2 = ld32(w + 8);
    const uint32_t d3 = ld32(w + 12), sh = (bq >> R8_SHIFT_LSB) & 3u, e = (bq >> R8_E_LSB) & 3u;
    const uint32_t rot = (bq >> R8_ROT_LSB) & 3u;
    CHECK(rot < 3 && (direct || !rot), "direct-only flags on a padded source");
    if (rot == 1) {
        d0 = d1;
        d1 = d2;
        d2 = d3;
    } else if (rot == 2) {
        d0 = d2;
        d1 = d3;
    }
    const uint32_t r0 = alignbyte(d1, d0, sh), r1 = alignbyte(d2, d1, sh), r2 = alignbyte(d3, d2, sh), r3 = alignbyte(d3, d3, sh);
    uint32_t lo1 = alignbyte(r2, r1, e), hi1 = alignbyte(r3, r2, e);
    if (bq & R8_SHARE) {
        lo1 = r0;
        hi1 = r1;
    }
    const uint32_t s[8] = {sel[0].x, sel[0].y, sel[0].z, sel[0].w, sel[1].x, sel[1].y, sel[1].z, sel[1].w};
    const uint32_t wv[8] = {wt[0].x, wt[0].y, wt[0].z, wt[0].w, wt[1].x, wt[1].y, wt[1].z, wt[1].w};
    for (int k = 0; k < 8; k++)
        t[k] = (int)dot2(k < 4 ? perm(r1, r0, s[k]) : perm(hi1, lo1, s[k]), wv[k]);
}

// does ANY window of the 8-pixel form hold the taps of this item?  (independent of the rule resize_items8 uses)
static bool fits8_anyhow(const int cl[8], const int cr[8], int row_len, bool direct)
{
    for (int wbase = 0; wbase + 16 <= row_len; wbase += 4)
        for (int rot = 0; rot <= (direct && wbase == row_len - 16 ? 2 : 0); rot++)
            for (int sh = 0; sh < 4; sh++)
                for (int e = 0; e < 4; e++)
                    for (int share = 0; share <= 1; share++) {
                        const int R = wbase + sh + 4 * rot, P[2] = {R, share ? R : R + 4 + e};
                        bool fit = true;
                        for (int k = 0; k < 8 && fit; k++)
                            fit = cl[k] >= P[k >> 2] && cr[k] <= P[k >> 2] + 7 && cr[k] < wbase + 16 && cr[k] >= cl[k];
                        if (fit)
                            return true;
                    }
    return false;
}

// slot by slot: the taps are those of the column the slot stands for, inside the window and the source row, and never
// decrease from one image column to the next (ring slots reflect: theirs run backwards); the 8-pixel form refused exactly
// where no window holds the taps
static void check_items(const ResizeTables &T, const ResizeLevel &L, int sw, int dw, int src_off, int row_len, bool direct)
{
    const XTab *xt = &T.xtab[L.xtab_off];
    if (L.fast4)
        for (int sdw = RESIZE_DW0; sdw < RESIZE_DW0 + resize_ndw(dw); sdw++) {
            const uint32_t bq = T.strip[L.rs_off + sdw].base_q;
            const int wbase = (int)(bq & 0xFFFFu), sh = (int)((bq >> 16) & 3u), edge = (int)((bq >> 18) & 1u);
            CHECK(direct || !edge, "edge flag on a padded source");
            CHECK(wbase >= 0 && wbase % 4 == 0 && wbase + 12 <= row_len, "4-px window %d..%d of a row of %d bytes", wbase, wbase + 11, row_len);
            const RsQuad &q = T.sel[L.rs_off + sdw];
            const uint32_t s[4] = {q.x, q.y, q.z, q.w};
            int prev = -1;
            for (int k = 0; k < 4; k++) {
                const int col = slot_column(sdw * 4 + k - RS_EDGE, dw);
                const int ps = wbase + sh + (edge ? 4 : 0);
                const int tl = ps + (int)(s[k] & 7u), tr = ps + (int)((s[k] >> 16) & 7u);
                CHECK(tl >= wbase && tr < wbase + 12 && tl >= src_off && tr < src_off + sw && tr >= tl, "4-px dword %d slot %d outside", sdw, k);
                if (col < 0)
                    continue;
                CHECK(tl == xt[col].sx + src_off && tr == xt[col].sx1 + src_off, "4-px dword %d slot %d: taps %d,%d for column %d", sdw, k, tl, tr, col);
                if (col == sdw * 4 + k - RS_EDGE) {  // an image column
                    CHECK(tl >= prev, "4-px dword %d: taps decrease", sdw);
                    prev = tl;
                }
            }
        }
    bool all_fit = true;
    for (int i = 0; i < resize_n8(dw); i++) {
        int cl[8], cr[8];
        for (int k = 0; k < 8; k++) {
            const XTab &x = xt[rs_slot_column(RESIZE_DW0 + 2 * i + (k >> 2), k & 3, dw)];
            cl[k] = x.sx + src_off;
            cr[k] = x.sx1 + src_off;
        }
        const bool any = fits8_anyhow(cl, cr, row_len, direct);
        all_fit = all_fit && any;
        if (!L.fast8)
            continue;
        const uint32_t bq = T.item8[L.r8_off + i];
        const int wbase = (int)(bq & R8_BASE_MASK), sh = (int)((bq >> R8_SHIFT_LSB) & 3u), e = (int)((bq >> R8_E_LSB) & 3u);
        CHECK(wbase >= 0 && wbase % 4 == 0 && wbase + 16 <= row_len, "8-px window %d..%d of a row of %d bytes", wbase, wbase + 15, row_len);
        const int R = wbase + sh + 4 * (int)((bq >> R8_ROT_LSB) & 3u), P[2] = {R, (bq & R8_SHARE) ? R : R + 4 + e};
        const RsQuad *q = &T.sel8[2 * (size_t)(L.r8_off + i)];
        const uint32_t s[8] = {q[0].x, q[0].y, q[0].z, q[0].w, q[1].x, q[1].y, q[1].z, q[1].w};
        int prev = -1;
        for (int k = 0; k < 8; k++) {
            const int x = RESIZE_DW0 * 4 + 8 * i + k - RS_EDGE, col = slot_column(x, dw);
            const int tl = P[k >> 2] + (int)(s[k] & 7u), tr = P[k >> 2] + (int)((s[k] >> 16) & 7u);
            CHECK(tl >= wbase && tr < wbase + 16 && tl >= src_off && tr < src_off + sw && tr >= tl, "8-px item %d slot %d outside", i, k);
            if (col < 0)
                continue;
            CHECK(tl == xt[col].sx + src_off && tr == xt[col].sx1 + src_off, "8-px item %d slot %d: taps %d,%d for column %d", i, k, tl, tr, col);
            if (col == x) {  // an image column
                CHECK(tl >= prev, "8-px item %d: taps decrease", i);
                prev = tl;
            }
        }
    }
    // (the 4-pixel form and non-negative row weights are further conditions of the 8-pixel form)
    CHECK(L.fast8 == (all_fit && L.fast4 && L.rows_pos), "8-pixel form %s although its taps %s", L.fast8 ? "taken" : "refused", all_fit ? "fit" : "do not fit");
}

int main(int argc, char **argv)
{
    CHECK(argc == 7, "usage: %s W H SCALE MAXLEVELS IMAGE OUT", argv[0]);
    const int w = atoi(argv[1]), h = atoi(argv[2]), maxl = atoi(argv[4]);
    const float sf = (float)atof(argv[3]);
    // the caller's image in an allocation of exactly w x h bytes
    std::vector<uint8_t> *img = new std::vector<uint8_t>((size_t)w * h);
    FILE *fi = fopen(argv[5], "rb");
    CHECK(fi && fread(img->data(), 1, img->size(), fi) == img->size(), "cannot read %s", argv[5]);
    fclose(fi);
    // level sizes as ORBextractor.cc:410-470 / :1112 make them
    std::vector<int> lw, lh;
    float scale = 1.0f;
    for (int l = 0; l < maxl; l++) {
        if (l > 0)
            scale = (float)((double)scale * (double)sf);
        const float inv = 1.0f / scale;
        const int ww = cv_round_host((float)w * inv), hh = cv_round_host((float)h * inv);
        if (ww < 62 || hh < 62)
            break;
        lw.push_back(ww);
        lh.push_back(hh);
    }
    const int nl = (int)lw.size();
    CHECK(nl >= 2, "no second level");
    ResizeTables T;
    std::vector<Plane> planes;
    planes.emplace_back(lw[0], lh[0]);
    for (int y = 0; y < h; y++)
        memcpy(planes[0].at(0, y), img->data() + (size_t)y * w, (size_t)w);
    FILE *fo = fopen(argv[6], "wb");
    CHECK(fo, "cannot write %s", argv[6]);
    std::vector<int> fast8;
    int direct8 = 0;
    for (int l = 1; l < nl; l++) {
        planes.emplace_back(lw[l], lh[l]);
        const Plane &S = planes[l - 1];
        Plane &D = planes[l];
        const ResizeLevel L = resize_add_level(T, S.w, S.h, S.pitch, D.w, D.h, D.pitch);
        CHECK(L.fast4 || sf > 1.5f, "level %d does not take the 4-pixel form", l);
        check_items(T, L, S.w, D.w, RS_EDGE, S.pitch, false);
        if (L.fast8)
            fast8.push_back(l);
        const XTab *xt = &T.xtab[L.xtab_off];
        const YTab *yt = &T.ytab[L.ytab_off];
        // the plain formula (k_resize_level) on the interior
        for (int y = 0; y < D.h; y++) {
            const uint8_t *S0 = S.row0(yt[y].sy0) + RS_EDGE, *S1 = S.row0(yt[y].sy1) + RS_EDGE;
            const YRow &yr = T.yrow[L.yrow_off + RS_EDGE + y];
            CHECK(yr.sy0 == yt[y].sy0 && yr.sy1 == yt[y].sy1 && yr.b0 == yt[y].b0 && yr.b1 == yt[y].b1, "row table, row %d", y);
            CHECK(yt[y].sy0 < S.h && yt[y].sy1 < S.h, "row taps of row %d", y);
            for (int x = 0; x < D.w; x++) {
                const int t0 = S0[xt[x].sx] * xt[x].a0 + S0[xt[x].sx1] * xt[x].a1;
                const int t1 = S1[xt[x].sx] * xt[x].a0 + S1[xt[x].sx1] * xt[x].a1;
                *D.at(x, y) = (uint8_t)vertical(yt[y].b0, yt[y].b1, t0, t1);
            }
        }
        // both forms, from the padded source plane (its border is 0xA5) and -- level 1 -- from the image itself
        ResizeLevel LD;
        const bool direct = l == 1 && w % 8 == 0 && w >= 64 && L.fast4;
        if (direct) {
            LD = resize_add_direct(T, L, S.w, D.w, D.pitch);
            CHECK(LD.fast4, "level 1 does not take the direct 4-pixel form");
            check_items(T, LD, S.w, D.w, 0, S.w, true);
            direct8 = LD.fast8 ? 1 : 0;
        }
        for (int src = 0; src < (direct ? 2 : 1); src++) {
            const ResizeLevel &U = src ? LD : L;
            for (int y = 0; y < D.h; y++) {
                const uint8_t *R0 = src ? img->data() + (size_t)yt[y].sy0 * w : S.row0(yt[y].sy0);
                const uint8_t *R1 = src ? img->data() + (size_t)yt[y].sy1 * w : S.row0(yt[y].sy1);
                if (U.fast4)
                    for (int sdw = RESIZE_DW0; sdw < RESIZE_DW0 + resize_ndw(D.w); sdw++) {
                        int t0[4], t1[4];
                        h4(R0, T.strip[U.rs_off + sdw].base_q, T.sel[U.rs_off + sdw], T.wt[U.rs_off + sdw], src != 0, t0);
                        h4(R1, T.strip[U.rs_off + sdw].base_q, T.sel[U.rs_off + sdw], T.wt[U.rs_off + sdw], src != 0, t1);
                        for (int k = 0; k < 4; k++) {
                            const int x = sdw * 4 + k - RS_EDGE, col = slot_column(x, D.w);
                            if (col >= 0)
                                CHECK(vertical(yt[y].b0, yt[y].b1, t0[k], t1[k]) == *D.at(col, y), "4-px form, source %d, level %d pixel (%d, %d)", src, l, x, y);
                        }
                    }
                if (U.fast8)
                    for (int i = 0; i < resize_n8(D.w); i++) {
                        int t0[8], t1[8];
                        h8(R0, T.item8[U.r8_off + i], &T.sel8[2 * (size_t)(U.r8_off + i)], &T.wt8[2 * (size_t)(U.r8_off + i)], src != 0, t0);
                        h8(R1, T.item8[U.r8_off + i], &T.sel8[2 * (size_t)(U.r8_off + i)], &T.wt8[2 * (size_t)(U.r8_off + i)], src != 0, t1);
                        for (int k = 0; k < 8; k++) {
                            const int x = RESIZE_DW0 * 4 + 8 * i + k - RS_EDGE, col = slot_column(x, D.w);
                            CHECK(yt[y].b0 >= 0 && yt[y].b1 >= 0, "negative row weight in the 8-pixel form");
                            if (col >= 0)
                                CHECK(vertical(yt[y].b0, yt[y].b1, t0[k], t1[k]) == *D.at(col, y), "8-px form, source %d, level %d pixel (%d, %d)", src, l, x, y);
                        }
                    }
            }
        }
        for (int y = 0; y < D.h; y++)
            CHECK(fwrite(D.at(0, y), 1, (size_t)D.w, fo) == (size_t)D.w, "short write");
    }
    fclose(fo);
    delete img;
    // every ring column lies in a dword the forms write
    for (int l = 1; l < nl; l++)
        CHECK(RESIZE_DW0 * 4 <= RS_EDGE - RS_RING && (RESIZE_DW0 + resize_ndw(lw[l])) * 4 > RS_EDGE + lw[l] - 1 + RS_RING &&
                  (RESIZE_DW0 + 2 * resize_n8(lw[l])) * 4 <= planes[l].pitch, "dword columns of level %d", l);
    printf("levels %d fast8", nl);
    for (int l : fast8)
        printf(" %d", l);
    printf(" direct8 %d\nresize_tables_test ok\n", direct8);
    return 0;
}
