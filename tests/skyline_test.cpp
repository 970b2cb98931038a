// csrc/skyline.h on the host: the reverse Cuthill-McKee order, the envelope layout and skyline_llt_solve against the dense
// llt_solve of opt_math.h on the permuted matrix, bit for bit, with 1, 2 and 5 cooperating threads.  Built by
// tests/test_skyline.py with -ffp-contract=off and the sanitizers; prints one line per check and exits non-zero on a miss.
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <thread>
#include <utility>
#include <vector>

#include "skyline.h"

using namespace orbgpu;

namespace {

constexpr int B = 7;
int failures = 0;

void check(bool ok, const char *graph, const char *what)
{
    printf("%s %s: %s\n", ok ? "ok" : "FAIL", graph, what);
    failures += ok ? 0 : 1;
}

struct Rng {
    uint64_t s;
    double next()  // uniform in (-1, 1)
    {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (double)(int64_t)(s >> 11) / (double)(1ull << 52) - 1.0;
    }
};

struct ThreadBarrier {
    std::mutex m;
    std::condition_variable cv;
    int waiting = 0, generation = 0, nt;
    explicit ThreadBarrier(int n) : nt(n) {}
    void wait()
    {
        std::unique_lock<std::mutex> lock(m);
        const int g = generation;
        if (++waiting == nt) {
            waiting = 0;
            generation++;
            cv.notify_all();
        } else {
            cv.wait(lock, [&] { return g != generation; });
        }
    }
};
struct BarrierRef {
    ThreadBarrier *b;
    void operator()() const { b->wait(); }
};

struct Graph {
    const char *name;
    int nv;
    std::vector<std::pair<int, int>> edges;
};

Graph chain(int n)
{
    Graph g{"chain", n, {}};
    for (int i = 0; i + 1 < n; i++)
        g.edges.push_back({i, i + 1});
    return g;
}

Graph ring(const char *name, int n, int reach)
{
    Graph g{name, n, {}};
    for (int i = 0; i < n; i++)
        for (int d = 1; d <= reach; d++)
            g.edges.push_back({i, (i + d) % n});
    return g;
}

struct System {
    int n = 0, bandwidth_blocks = 0;
    int64_t envelope = 0;
    std::vector<int32_t> order, first, last;
    std::vector<int64_t> off;
    std::vector<double> dense, sky, b;  // dense: the permuted matrix, lower triangle packed by tri_at
};

// H = sum over edges of (Ji Jj)'(Ji Jj) plus a small block per vertex, in the RCM order
System build(const Graph &g, uint64_t seed, bool &is_permutation)
{
    System S;
    const int nv = g.nv;
    std::vector<std::vector<int32_t>> nb((size_t)nv);
    for (auto &e : g.edges) {
        if (std::find(nb[e.first].begin(), nb[e.first].end(), e.second) == nb[e.first].end()) {
            nb[e.first].push_back(e.second);
            nb[e.second].push_back(e.first);
        }
    }
    std::vector<int32_t> start((size_t)nv + 1, 0), adj;
    for (int v = 0; v < nv; v++) {
        adj.insert(adj.end(), nb[v].begin(), nb[v].end());
        start[v + 1] = (int32_t)adj.size();
    }
    S.order.assign((size_t)nv, -1);
    rcm_order(nv, start.data(), adj.data(), S.order.data());
    std::vector<int32_t> pos((size_t)nv, -1);
    is_permutation = true;
    for (int p = 0; p < nv; p++) {
        const int v = S.order[p];
        if (v < 0 || v >= nv || pos[v] >= 0)
            is_permutation = false;
        else
            pos[v] = p;
    }
    if (!is_permutation)
        return S;
    std::vector<int32_t> first_block((size_t)nv);
    for (int v = 0; v < nv; v++) {
        int f = pos[v];
        for (int w : nb[v])
            f = std::min(f, (int)pos[w]);
        first_block[pos[v]] = f;
        S.bandwidth_blocks = std::max(S.bandwidth_blocks, pos[v] - f + 1);
    }
    const int n = S.n = B * nv;
    S.first.assign((size_t)n, 0), S.last.assign((size_t)n, 0), S.off.assign((size_t)n, 0);
    S.envelope = skyline_layout(nv, B, first_block.data(), S.first.data(), S.off.data(), S.last.data());
    std::vector<double> full((size_t)n * n, 0.0);
    Rng rng{seed};
    auto add = [&](int a, const double *Ja, int c, const double *Jc) {  // block (a, c) += Ja' Jc
        for (int x = 0; x < B; x++)
            for (int y = 0; y < B; y++)
                for (int r = 0; r < B; r++)
                    full[(size_t)(B * a + x) * n + (B * c + y)] += Ja[B * r + x] * Jc[B * r + y];
    };
    double Ji[B * B], Jj[B * B];
    for (auto &e : g.edges) {
        for (int k = 0; k < B * B; k++)
            Ji[k] = rng.next(), Jj[k] = rng.next();
        const int a = pos[e.first], c = pos[e.second];
        add(a, Ji, a, Ji), add(c, Jj, c, Jj), add(a, Ji, c, Jj), add(c, Jj, a, Ji);
    }
    for (int v = 0; v < nv; v++) {
        for (int k = 0; k < B * B; k++)
            Ji[k] = rng.next();
        add(v, Ji, v, Ji);
        for (int x = 0; x < B; x++)
            full[(size_t)(B * v + x) * n + (B * v + x)] += 0.5;
    }
    S.dense.assign(tri_at(n, 0), 0.0);
    S.sky.assign((size_t)S.envelope, 0.0);
    for (int i = 0; i < n; i++)
        for (int k = 0; k <= i; k++) {
            S.dense[tri_at(i, k)] = full[(size_t)i * n + k];
            if (k >= S.first[i])
                S.sky[(size_t)(S.off[i] + k)] = full[(size_t)i * n + k];
            else if (full[(size_t)i * n + k] != 0.0)
                is_permutation = false;  // a non-zero outside the envelope: the layout is wrong
        }
    S.b.resize((size_t)n);
    for (double &v : S.b)
        v = rng.next();
    return S;
}

bool solve_sky(const System &S, int nt, std::vector<double> &A, std::vector<double> &x)
{
    A = S.sky, x = S.b;
    std::vector<double> work(2 * (size_t)S.n + 1);
    if (nt == 1)
        return skyline_llt_solve(S.n, S.first.data(), S.off.data(), S.last.data(), A.data(), x.data(), work.data(), 0, 1,
                                 NoBarrier{});
    ThreadBarrier bar(nt);
    std::vector<char> ok((size_t)nt, 0);
    std::vector<std::thread> th;
    for (int t = 0; t < nt; t++)
        th.emplace_back([&, t] {
            ok[t] = skyline_llt_solve(S.n, S.first.data(), S.off.data(), S.last.data(), A.data(), x.data(), work.data(), t, nt,
                                      BarrierRef{&bar});
        });
    for (auto &t : th)
        t.join();
    for (int t = 1; t < nt; t++)
        if (ok[t] != ok[0])
            failures++;
    return ok[0] != 0;
}

bool same_bits(const double *a, const double *b, size_t n)
{
    return n == 0 || memcmp(a, b, n * sizeof(double)) == 0;
}

void run(const Graph &g, uint64_t seed)
{
    bool perm = false;
    System S = build(g, seed, perm);
    check(perm, g.name, "the order is a permutation and nothing lies outside the envelope");
    if (!perm)
        return;
    printf("info %s: n %d envelope %lld bandwidth_blocks %d\n", g.name, S.n, (long long)S.envelope, S.bandwidth_blocks);
    std::vector<double> D = S.dense, xd = S.b, work(2 * (size_t)S.n + 1);
    const bool okd = llt_solve(S.n, D.data(), xd.data(), work.data(), 0, 1, NoBarrier{});
    check(okd || S.n == 0, g.name, "the dense factorisation succeeds");
    for (int nt : {1, 2, 5}) {
        std::vector<double> A, x;
        const bool ok = solve_sky(S, nt, A, x);
        bool same = ok == okd && same_bits(x.data(), xd.data(), (size_t)S.n);
        for (int i = 0; i < S.n && same; i++)
            for (int k = S.first[i]; k <= i && same; k++)
                same = same_bits(&A[(size_t)(S.off[i] + k)], &D[tri_at(i, k)], 1);
        char what[96];
        snprintf(what, sizeof what, "x and every kept entry of L equal the dense ones bit for bit, %d thread(s)", nt);
        check(same, g.name, what);
    }
    if (S.n == 0)
        return;
    // a pivot that is not > 0: false and x = 0, as the dense solve
    System Bad = S;
    const int j = S.n / 2;
    Bad.sky[(size_t)(Bad.off[j] + j)] = -1.0;
    D = S.dense, xd = S.b;
    D[tri_at(j, j)] = -1.0;
    const bool okd2 = llt_solve(S.n, D.data(), xd.data(), work.data(), 0, 1, NoBarrier{});
    for (int nt : {1, 5}) {
        std::vector<double> A, x;
        const bool ok = solve_sky(Bad, nt, A, x);
        bool zero = !ok && !okd2;
        for (int i = 0; i < S.n; i++)
            zero = zero && x[i] == 0.0 && xd[i] == 0.0;
        check(zero, g.name, nt == 1 ? "a non-positive pivot gives false and x = 0, 1 thread"
                                    : "a non-positive pivot gives false and x = 0, 5 threads");
    }
    Bad = S;
    Bad.sky[(size_t)(Bad.off[j] + j)] = std::nan("");
    std::vector<double> A, x;
    check(!solve_sky(Bad, 1, A, x) && x[0] == 0.0 && x[S.n - 1] == 0.0, g.name, "a NaN pivot gives false and x = 0");
}

} // namespace

int main()
{
    run(chain(9), 1);
    run(ring("ring", 12, 1), 2);
    {
        Graph g = ring("ring_with_chords", 16, 1);
        g.edges.push_back({0, 8}), g.edges.push_back({3, 11}), g.edges.push_back({5, 6}), g.edges.push_back({1, 13});
        run(g, 3);
    }
    {
        Graph g = chain(5);
        g.name = "two_components";
        g.nv = 12;
        for (int i = 5; i < 12; i++)
            g.edges.push_back({i, 5 + (i - 5 + 1) % 7});
        run(g, 4);
    }
    run(Graph{"single_block", 1, {}}, 5);
    run(Graph{"empty", 0, {}}, 6);
    {
        // A ring of 64 with neighbours at +-1 and +-2: every degree is 4, so the start is row 0 and a breadth-first level
        // holds 2 arcs x 2 vertices, in the slots (2k - 1, 2k, 64 - 2k, 65 - 2k).  A vertex is linked to its own slot of the
        // next level (4 positions on) and, on the descending arc, slot 2 also to slot 3 of the next level: 2 x 2 + 1
        // positions.  So the bandwidth -- the largest |position(i) - position(j)| over the blocks that are not zero -- is
        // at most 2 x 2 + 1 blocks, and the longest block row, diagonal included, one more.
        Graph g = ring("ring64_reach2", 64, 2);
        bool perm = false;
        System S = build(g, 7, perm);
        check(perm && S.bandwidth_blocks - 1 <= 2 * 2 + 1, g.name, "bandwidth at most 2 x 2 + 1 blocks off the diagonal");
        run(g, 7);
    }
    printf("%s\n", failures ? "FAILED" : "PASSED");
    return failures ? 1 : 0;
}
