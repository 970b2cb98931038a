// k_orient finds the level of a selection slot through slot_level() (extractor_plan.h) and the byte table the plan builds
// from it (t_slot_level).  For every plan on a grid of image sizes, feature counts and level counts: the levels' slot
// ranges tile [0, sel_cap_total) without gap or overlap, and function and table name for every slot the one level whose
// range holds it.  Host-only: g++ -std=c++17, no HIP (tests/test_orient_levels.py builds and runs it, plain and under
// AddressSanitizer + UBSan).
#include <cstdio>
#include <cstdlib>
#include <string>

#include "extractor_plan.h"

using namespace orbgpu;

static int g_failed = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            printf("FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); \
            printf(__VA_ARGS__);                          \
            printf("\n");                                 \
            g_failed++;                                   \
        }                                                 \
    } while (0)

static void check_plan(const ExtractorPlan &P, int w, int h, int nfeatures, int nl)
{
    const std::vector<LevelGeom> &geom = P.geom;
    CHECK((int)geom.size() == nl, "%dx%d n%d l%d", w, h, nfeatures, nl);
    // the ranges: contiguous, ascending from 0, none empty, sel_cap_total in all
    int end = 0;
    for (int l = 0; l < nl; l++) {
        CHECK(geom[l].sel_off == end && geom[l].sel_cap > 0, "%dx%d n%d l%d: level %d starts at %d, the one below ends at %d", w, h,
              nfeatures, nl, l, geom[l].sel_off, end);
        end = geom[l].sel_off + geom[l].sel_cap;
    }
    CHECK(end == P.sel_cap_total, "%dx%d n%d l%d: ranges end at %d of %d", w, h, nfeatures, nl, end, P.sel_cap_total);
    CHECK(P.count<uint8_t>(P.t_slot_level) == (size_t)P.sel_cap_total && P.t_slot_level.off % PLAN_ALIGN == 0 &&
              P.t_slot_level.off + P.t_slot_level.bytes <= P.blob.size(),
          "%dx%d n%d l%d: table of %zu bytes", w, h, nfeatures, nl, P.t_slot_level.bytes);
    const uint8_t *tab = P.table<uint8_t>(P.t_slot_level);
    for (int slot = 0; slot < P.sel_cap_total; slot++) {
        int holders = 0, level = -1;  // by definition: every level whose range holds the slot
        for (int l = 0; l < nl; l++)
            if (geom[l].sel_off <= slot && slot < geom[l].sel_off + geom[l].sel_cap) {
                holders++;
                level = l;
            }
        CHECK(holders == 1, "%dx%d n%d l%d: slot %d lies in %d ranges", w, h, nfeatures, nl, slot, holders);
        CHECK(slot_level(geom, slot) == level, "%dx%d n%d l%d: slot %d: function %d, range %d", w, h, nfeatures, nl, slot,
              slot_level(geom, slot), level);
        CHECK((int)tab[slot] == level, "%dx%d n%d l%d: slot %d: table %d, range %d", w, h, nfeatures, nl, slot, (int)tab[slot], level);
    }
    CHECK(slot_level(geom, -1) == -1 && slot_level(geom, P.sel_cap_total) == -1 && slot_level(geom, P.sel_cap_total + 7) == -1,
          "%dx%d n%d l%d: slots outside every range", w, h, nfeatures, nl);
}

int main()
{
    static const int sizes[][2] = {{64, 64}, {96, 80}, {176, 144}, {200, 103}, {640, 480}, {1280, 960}};
    static const int features[] = {9, 37, 200, 1000, 2000};
    int plans = 0;
    for (const auto &s : sizes)
        for (int nfeatures : features) {
            int planned = 0;
            for (int nl = 1; nl <= 8; nl++) {  // every level count the size allows at scale 1.2
                ExtractorConsts cst;
                ExtractorPlan P;
                std::string why;
                if (build_consts(nfeatures, 1.2f, nl, &cst, &why) != ORBGPU_OK ||
                    plan_extractor(cst, s[0], s[1], PlanHooks(), &P, &why) != ORBGPU_OK)
                    continue;
                check_plan(P, s[0], s[1], nfeatures, nl);
                planned++;
                plans++;
                printf("P %dx%d n%d l%d slots %d\n", s[0], s[1], nfeatures, nl, P.sel_cap_total);
            }
            if (!planned) {  // (a size the plan refuses at every level count has no slots to check)
                ExtractorConsts cst;
                ExtractorPlan P;
                std::string why;
                if (build_consts(nfeatures, 1.2f, 1, &cst, &why) == ORBGPU_OK)
                    plan_extractor(cst, s[0], s[1], PlanHooks(), &P, &why);
                printf("R %dx%d n%d %s\n", s[0], s[1], nfeatures, why.c_str());
            }
        }
    ExtractorPlan none;
    CHECK(slot_level(none.geom, 0) == -1, "a plan without levels");
    printf("%d plans\n", plans);
    if (g_failed)
        return 1;
    printf("orient_levels_test ok\n");
    return 0;
}
