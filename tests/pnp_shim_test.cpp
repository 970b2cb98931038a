// PnPsolverT (orbgpu_shim.hpp) without a device: the sampler replay over a scripted RandomInt, and the state the class
// carries between iterate calls, with the library call replaced (SetSolver) by a scan over injected counts.  Arguments:
// in.bin out.bin.  in.bin: int32 n1, min_inliers, max_iterations, chunk, K, Hc, calls; int32 valid[n1]; int32 rand[K] (the
// values RandomInt returns, in call order); int32 counts[Hc]; int32 refined[Hc] (the refined count of hypothesis h).
// out.bin: int32 N, adjusted min_inliers, max_its; per iterate(chunk) call, `calls` of them or until bNoMore: int32 returned
// (1 / 0), nInliers, bNoMore, iterations, popcount of vbInliers, (int32) Tcw[0] or -1, n_hyp the library was asked for;
// then int32 -1, the number of sets drawn, and the sets.  For tests/test_pnp_shim.py to compare with tests/pnp_model.py.
#include <fstream>
#include <iostream>
#include <iterator>

#include "pnp_standin.hpp"

using namespace ORB_SLAM2;

int main(int argc, char **argv)
{
    if (argc != 3) {
        std::cerr << "usage: pnp_shim_test in.bin out.bin\n";
        return 2;
    }
    std::ifstream f(argv[1], std::ios::binary);
    const std::vector<char> buf((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    const int32_t *p = reinterpret_cast<const int32_t *>(buf.data());
    const int n1 = p[0], min_inliers = p[1], max_iterations = p[2], chunk = p[3], K = p[4], Hc = p[5], calls = p[6];
    const int32_t *valid = p + 7, *rnd = valid + n1, *counts = rnd + K, *refined = counts + Hc;
    Frame F;
    F.mvKeysUn.resize(n1);
    F.mvLevelSigma2.assign(8, 1.f);
    F.fx = F.fy = 500.f, F.cx = 320.f, F.cy = 240.f;
    std::vector<MapPoint> mps(n1);
    std::vector<MapPoint *> matches(n1, nullptr);
    for (int i = 0; i < n1; i++) {
        mps[i].mWorldPos.create(3, 1, CV_32F);
        mps[i].mWorldPos.ptr<float>()[0] = (float)i, mps[i].mWorldPos.ptr<float>()[1] = 1.f, mps[i].mWorldPos.ptr<float>()[2] = 5.f;
        F.mvKeysUn[i].octave = i % 8;
        // the two ways a row is dropped, in turn
        if (valid[i])
            matches[i] = &mps[i];
        else if (i % 2)
            matches[i] = &mps[i], mps[i].mbBad = true;
    }
    int at = 0, asked = 0;
    try {
        PnPsolver solver(
            F, matches, [](MapPoint *mp) { return mp->mWorldPos.ptr<float>(); }, [&](int, int) { return at < K ? rnd[at++] : 0; });
        solver.SetRansacParameters(0.99, min_inliers, max_iterations, 4, 0.5f, 5.991f);
        const int mi = solver.MinInliers(), max_its = solver.MaxIterations(), N = solver.NumCorrespondences();
        // P8 over the injected counts: hypothesis h has its first counts[h] rows set, its Refine the first refined[h]
        solver.SetSolver([&](const orbgpu_pnp_problem *q, int32_t *c, float *T, uint64_t *masks, uint64_t *rm, orbgpu_pnp_result *r) {
            const int H = q->n_hyp, words = (q->n1 + 63) / 64;
            asked = H;
            if (H > Hc || !q->sets || q->n1 != n1 || q->min_set != 4)
                return (int)ORBGPU_EINVAL;
            std::memset(r, 0, sizeof(*r));
            for (int h = 0; h < H; h++) {
                c[h] = counts[h], T[16 * h] = (float)h;
                for (int i = 0; i < counts[h] && i < n1; i++)
                    masks[(size_t)h * words + i / 64] |= 1ull << (i % 64);
            }
            int it = q->start_iteration, best = q->best_so_far, best_it = -1, cur = 0;
            r->accepted = -1;
            while ((it < max_its || cur < q->n_iterations) && it < H) {
                cur++;
                const int h = it++;
                if (c[h] >= mi && c[h] > best) {
                    best = c[h], best_it = h;
                    if (refined[h] > mi) {
                        r->accepted = h, r->n_inliers = refined[h], r->Tcw[0] = (float)(1000 + h);
                        for (int i = 0; i < refined[h] && i < n1; i++)
                            rm[i / 64] |= 1ull << (i % 64);
                        break;
                    }
                }
            }
            r->no_more = r->accepted < 0 && !(it < max_its || cur < q->n_iterations);
            r->n = N, r->min_inliers = mi, r->max_its = max_its, r->best_inliers = best, r->best_iteration = best_it, r->iterations = it;
            return (int)ORBGPU_OK;
        });
        std::ofstream o(argv[2], std::ios::binary);
        auto put = [&o](int32_t v) { o.write(reinterpret_cast<const char *>(&v), 4); };
        put(N), put(mi), put(max_its);
        bool no_more = false;
        for (int call = 0; call < calls && !no_more; call++) {
            std::vector<bool> inl;
            int n_inl = 0;
            asked = 0;
            const float *T = solver.iterate(chunk, no_more, inl, n_inl);
            int pop = 0;
            for (bool b : inl)
                pop += b;
            put(T != nullptr), put(n_inl), put(no_more), put(solver.Iterations()), put(pop), put(T ? (int32_t)T[0] : -1), put(asked);
        }
        put(-1), put((int32_t)(solver.Sets().size() / 4));
        for (int32_t v : solver.Sets())
            put(v);
    } catch (const std::exception &e) {
        std::cerr << e.what() << "\n";
        return 1;
    }
    std::cout << "pnp shim ok\n";
    return 0;
}
