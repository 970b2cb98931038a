// bf_select.h on the CPU: the order walk k_bf_topk's selection runs now against the blanking loop it ran before, for one
// lane and one row block at a time.  Lists, bars and trip counts must be equal.
//   - every block whose 16 distances are each one of bar - 1, bar, bar + 1 (3^16 blocks: every subset of hits, every
//     pattern of ties among them), into an empty list;
//   - crafted blocks: ties (the lower register first), 16 equal distances (16 trips, then "none left"), all 16 past
//     jlast, distances above 128 (negative dot) next to hits, a list that fills in the middle of a block, rows past
//     jlast between two valid ones;
//   - random sequences of blocks into one lane (the list and the bar carry over as from tile to tile), distances drawn
//     round the bar, random jlast; where the lane started empty the list is also compared with the 4 smallest keys of
//     everything within the first bar;
//   - random sequences into the two lanes of an A row, with and without one bar for both (share_bar, which the kernel
//     does not do: see bf_select.h): the merged lists are equal.
// Prints "bf_select_test ok <blocks>" and returns 0, or the first mismatch and 1.
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <thread>
#include <vector>

#include "bf_select.h"

using namespace orbgpu_bfsel;

static std::atomic<int> g_bad{0};

static inline int tagged(int ham, int reg) { return (256 - 2 * ham) * 16 + (15 - reg); }

static void report(const char *what, const int acc[16], const Lane &before, int j0, int jlast, const Lane &a, int ta,
                   const Lane &b, int tb)
{
    if (g_bad.fetch_add(1) != 0)
        return;
    std::fprintf(stderr, "mismatch (%s): j0 %d jlast %d bar %d list %08x %08x %08x %08x, distances", what, j0, jlast, before.lim,
                 before.t[0], before.t[1], before.t[2], before.t[3]);
    for (int reg = 0; reg < 16; reg++)
        std::fprintf(stderr, " %d", (256 - (acc[reg] >> 4)) / 2);
    std::fprintf(stderr, "\n  blanking: %d trips, bar %d, list %08x %08x %08x %08x\n  order walk: %d trips, bar %d, list %08x %08x %08x %08x\n",
                 ta, a.lim, a.t[0], a.t[1], a.t[2], a.t[3], tb, b.lim, b.t[0], b.t[1], b.t[2], b.t[3]);
}

// one block through both forms; L is advanced.  Returns the trips.
static inline int both(const int acc[16], Lane &L, int j0, int jlast, unsigned long long &n)
{
    n++;
    Lane a = L, b = L;
    const int ta = select_blanking(acc, a, j0, jlast);
    const int tb = select_order_walk(acc, b, j0, jlast);
    if (ta != tb || a.lim != b.lim || !std::equal(a.t, a.t + 4, b.t))
        report("forms differ", acc, L, j0, jlast, a, ta, b, tb);
    L = b;
    return tb;
}

// the 4 smallest keys of everything within the bar, straight from the definition
static void brute(const std::vector<uint32_t> &keys, uint32_t out[4])
{
    std::vector<uint32_t> k = keys;
    std::sort(k.begin(), k.end());
    for (int q = 0; q < 4; q++)
        out[q] = q < (int)k.size() ? k[q] : KEY_NONE;
}

static void expect(bool ok, const char *what)
{
    if (!ok && g_bad.fetch_add(1) == 0)
        std::fprintf(stderr, "crafted case failed: %s\n", what);
}

// blocks over {bar - 1, bar, bar + 1} whose three leading digits are `chunk` (27 chunks)
static unsigned long long exhaustive_chunk(int chunk)
{
    unsigned long long n = 0;
    const int dmax = 71, acc_min = 256 - 2 * dmax;
    int d[16], acc[16];
    for (int k = 0; k < 13; k++)
        d[k] = 0;
    d[13] = chunk % 3, d[14] = chunk / 3 % 3, d[15] = chunk / 9;
    for (int k = 0; k < 16; k++)
        acc[k] = tagged(dmax - 1 + d[k], k);
    for (;;) {
        Lane L(acc_min);
        both(acc, L, 100, 4095, n);
        int k = 0;
        while (k < 13 && d[k] == 2) {
            d[k] = 0;
            acc[k] = tagged(dmax - 1, k);
            k++;
        }
        if (k == 13)
            break;
        d[k]++;
        acc[k] = tagged(dmax - 1 + d[k], k);
    }
    return n;
}

static unsigned long long crafted()
{
    unsigned long long n = 0;
    int acc[16];
    const int j0 = 64, far = 200;
    auto row = [&](int reg) { return j0 + (reg & 3) + 8 * (reg >> 2); };
    auto key = [&](int ham, int reg) { return (uint32_t)(ham << 12 | row(reg)); };
    auto fill = [&](int ham) {
        for (int reg = 0; reg < 16; reg++)
            acc[reg] = tagged(ham, reg);
    };
    {  // ties: registers 9, 3, 12 at distance 20, register 5 at 19: 5 first, then 3, 9, 12
        fill(far);
        acc[9] = tagged(20, 9), acc[3] = tagged(20, 3), acc[12] = tagged(20, 12), acc[5] = tagged(19, 5);
        Lane L(256 - 2 * 71);
        const int trips = both(acc, L, j0, 4095, n);
        expect(trips == 4 && L.t[0] == key(19, 5) && L.t[1] == key(20, 3) && L.t[2] == key(20, 9) && L.t[3] == key(20, 12) &&
                   L.lim == 256 - 2 * 20,
               "ties");
    }
    {  // 16 equal distances: 16 trips, then none left
        fill(0);
        Lane L(256 - 2 * 71);
        const int trips = both(acc, L, j0, 4095, n);
        expect(trips == 16 && L.t[0] == key(0, 0) && L.t[1] == key(0, 1) && L.t[2] == key(0, 2) && L.t[3] == key(0, 3) && L.lim == 256,
               "16 rows at distance 0");
        int m = max16(acc);
        for (int trip = 0; trip < 16; trip++) {
            uint32_t nn;
            const int next = next_below(acc, m, &nn);
            expect(((int)nn < 0) == (trip < 15) && (next == SENTINEL) == (trip == 15) && (trip == 15 || next == acc[trip + 1]),
                   "descending walk over 16 equal distances");
            m = next;
        }
    }
    {  // all 16 past jlast: 16 trips, nothing listed, the bar stays
        fill(3);
        Lane L(256 - 2 * 71);
        const int trips = both(acc, L, j0, j0 - 1, n);
        expect(trips == 16 && L.t[0] == KEY_NONE && L.lim == 256 - 2 * 71, "all past jlast");
    }
    {  // th_low 256: every distance is within the bar at first; 255 and 200 (negative dot) next to 10 and 130
        fill(256);
        acc[2] = tagged(255, 2), acc[7] = tagged(200, 7), acc[8] = tagged(10, 8), acc[15] = tagged(130, 15), acc[0] = tagged(129, 0);
        Lane L(256 - 2 * 256);
        const int trips = both(acc, L, j0, 4095, n);
        expect(trips == 4 && L.t[0] == key(10, 8) && L.t[1] == key(129, 0) && L.t[2] == key(130, 15) && L.t[3] == key(200, 7) &&
                   L.lim == 256 - 2 * 200,
               "negative dot");
        Lane E(256 - 2 * 256);  // alone: 255 and the eleven rows at 256 are hits of an empty list
        fill(256);
        acc[2] = tagged(255, 2);
        both(acc, E, j0, 4095, n);
        expect(E.t[0] == key(255, 2) && E.t[1] == key(256, 0) && E.t[2] == key(256, 1) && E.t[3] == key(256, 3), "distance 256");
    }
    {  // two entries listed already; the block adds 30, 40 (the list is full, bar 60 -> 50), then 45 passes, 55 does not
        fill(far);
        acc[1] = tagged(30, 1), acc[4] = tagged(40, 4), acc[6] = tagged(45, 6), acc[10] = tagged(55, 10), acc[11] = tagged(50, 11);
        Lane L(256 - 2 * 60);
        L.t[0] = 35u << 12 | 7, L.t[1] = 50u << 12 | 9;
        const int trips = both(acc, L, j0, 4095, n);
        // 30, 40 fill the list (bar 50); 45 pushes 50|9 out (bar 45); 50 and 55 are no hits any more
        expect(trips == 3 && L.t[0] == key(30, 1) && L.t[1] == (35u << 12 | 7) && L.t[2] == key(40, 4) && L.t[3] == key(45, 6) &&
                   L.lim == 256 - 2 * 45,
               "list fills in the middle of a block");
    }
    {  // registers 0..5 are rows j0 .. j0 + 3, j0 + 8, j0 + 9; jlast = j0 + 9.  Closest first: 1 (valid), 8 (past), 6 (past), 2 (valid)
        fill(far);
        acc[1] = tagged(5, 1), acc[8] = tagged(6, 8), acc[6] = tagged(7, 6), acc[2] = tagged(8, 2), acc[5] = tagged(9, 5);
        Lane L(256 - 2 * 71);
        const int trips = both(acc, L, j0, j0 + 9, n);
        expect(trips == 5 && L.t[0] == key(5, 1) && L.t[1] == key(8, 2) && L.t[2] == key(9, 5) && L.t[3] == KEY_NONE && L.lim == 256 - 2 * 71,
               "rows past jlast between two valid ones");
    }
    return n;
}

// sequences of blocks into one lane
static unsigned long long random_lane(uint64_t seed, int sequences)
{
    unsigned long long n = 0;
    std::mt19937_64 rng(seed);
    auto below = [&](int m) { return (int)(rng() % (uint64_t)m); };
    int acc[16];
    for (int it = 0; it < sequences; it++) {
        const int dmax = below(8) == 0 ? 256 : 20 + below(120), acc_min = 256 - 2 * dmax;
        const int blocks = 1 + below(8), h = below(2), jlast = below(4) == 0 ? below(32 * blocks + 1) - 1 : 4095;
        Lane L(acc_min);
        std::vector<uint32_t> within;
        for (int blk = 0; blk < blocks; blk++) {
            const int j0 = 32 * blk + 4 * h;
            const int mode = below(4);  // distances far from the bar, round the bar of the lane, few values, anything
            for (int reg = 0; reg < 16; reg++) {
                const int bar = (256 - L.lim) / 2;
                int ham = mode == 0 ? 100 + below(60) : mode == 1 ? bar - 2 + below(5) : mode == 2 ? bar - below(2) * below(3) : below(257);
                if (mode == 0 && below(6) == 0)
                    ham = below(dmax + 1);
                ham = ham < 0 ? 0 : ham > 256 ? 256 : ham;
                acc[reg] = tagged(ham, reg);
                const int j = j0 + (reg & 3) + 8 * (reg >> 2);
                if (ham <= dmax && j <= jlast)
                    within.push_back((uint32_t)(ham << 12 | j));
            }
            both(acc, L, j0, jlast, n);
        }
        uint32_t want[4];
        brute(within, want);
        if (!std::equal(want, want + 4, L.t) && g_bad.fetch_add(1) == 0)
            std::fprintf(stderr, "list differs from the 4 smallest keys: seed %llu sequence %d: %08x %08x %08x %08x, want %08x %08x %08x %08x\n",
                         (unsigned long long)seed, it, L.t[0], L.t[1], L.t[2], L.t[3], want[0], want[1], want[2], want[3]);
    }
    return n;
}

// the two lanes of an A row over the same tiles, bars apart and shared once per tile: the merged lists are equal
static unsigned long long random_pair(uint64_t seed, int sequences)
{
    unsigned long long n = 0;
    std::mt19937_64 rng(seed);
    auto below = [&](int m) { return (int)(rng() % (uint64_t)m); };
    int acc[2][2][16];
    for (int it = 0; it < sequences; it++) {
        const int dmax = below(8) == 0 ? 256 : 20 + below(120), acc_min = 256 - 2 * dmax;
        const int tiles = 1 + below(5), jlast = below(4) == 0 ? below(64 * tiles + 1) - 1 : 4095;
        Lane apart[2] = {Lane(acc_min), Lane(acc_min)}, shared[2] = {Lane(acc_min), Lane(acc_min)};
        const int rich = below(2);  // the half whose rows are close
        for (int tile = 0; tile < tiles; tile++) {
            for (int u = 0; u < 2; u++)
                for (int h = 0; h < 2; h++)
                    for (int reg = 0; reg < 16; reg++) {
                        const int near = below(h == rich ? 3 : 6) == 0;
                        const int ham = near ? below(dmax + 2) : 90 + below(80);
                        acc[u][h][reg] = tagged(ham > 256 ? 256 : ham, reg);
                    }
            share_bar(shared[0], shared[1]);
            for (int u = 0; u < 2; u++)
                for (int h = 0; h < 2; h++) {
                    const int j0 = 64 * tile + 32 * u + 4 * h;
                    both(acc[u][h], apart[h], j0, jlast, n);
                    both(acc[u][h], shared[h], j0, jlast, n);
                }
        }
        top4_merge(apart[0].t, apart[1].t);
        top4_merge(shared[0].t, shared[1].t);
        if (!std::equal(apart[0].t, apart[0].t + 4, shared[0].t) && g_bad.fetch_add(1) == 0)
            std::fprintf(stderr, "shared bar changes the merged list: seed %llu sequence %d\n", (unsigned long long)seed, it);
    }
    return n;
}

int main()
{
    const int jobs = 27 + 1 + 8 + 4;
    std::atomic<int> next{0};
    std::atomic<unsigned long long> total{0};
    unsigned nt = std::thread::hardware_concurrency();
    nt = nt < 1 ? 1 : nt > 8 ? 8 : nt;
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nt; t++)
        th.emplace_back([&] {
            for (int j; (j = next.fetch_add(1)) < jobs;)
                total += j < 27 ? exhaustive_chunk(j) : j == 27 ? crafted() : j < 36 ? random_lane(2000 + (uint64_t)j, 100000)
                                                                                     : random_pair(3000 + (uint64_t)j, 25000);
        });
    for (auto &t : th)
        t.join();
    if (g_bad.load()) {
        std::fprintf(stderr, "bf_select_test: %d checks failed\n", g_bad.load());
        return 1;
    }
    std::printf("bf_select_test ok %llu\n", total.load());
    return 0;
}
