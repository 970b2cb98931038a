// The graph of OptimizerT::OptimizeEssentialGraph (orbgpu_shim.hpp: EssentialGraphT) over stand-in key frames and map points
// from the file of tests/test_eg_shim.py; needs no device.  Arguments: in.txt out.txt (format of in.txt:
// tests/integration/eg_standin.hpp).  out.txt: V E M fix_scale n_iterations; rows[V] (key-frame indices); fixed[V]; Scw and
// Snc [8 V] as hex doubles; edge_i, edge_j, edge_kind [E]; points[M] (map-point indices); point_ref[M]; world_pos [3 M] as
// hex floats.
#include <cstdio>
#include <iostream>

#define ORBGPU_EG_SCENE
#include "eg_standin.hpp"

using namespace ORB_SLAM2;

int main(int argc, char **argv)
{
    if (argc != 3) {
        std::cerr << "usage: eg_shim_test in.txt out.txt\n";
        return 2;
    }
    try {
        EgScene sc(argv[1]);
        EssentialGraphAccess access;
        const orbgpu_shim::EssentialGraphT<KeyFrame, MapPoint> g(&sc.map, sc.pLoopKF, sc.pCurKF, sc.NonCorrectedSim3, sc.CorrectedSim3,
                                                                 sc.LoopConnections, access);
        const orbgpu_essential_graph_problem p = g.Problem(sc.bFixScale);
        FILE *o = fopen(argv[2], "w");
        if (!o)
            throw std::runtime_error("cannot write the output file");
        const int M = (int)g.points.size();
        fprintf(o, "%d %d %d %d %d\n", p.n_vertices, p.n_edges, M, p.fix_scale, p.n_iterations);
        for (KeyFrame *k : g.rows)
            fprintf(o, "%d ", sc.kf_index(k));
        for (int v = 0; v < p.n_vertices; v++)
            fprintf(o, "%d ", (int)p.fixed[v]);
        for (const double *S : {p.Scw, p.Snc})
            for (int v = 0; v < 8 * p.n_vertices; v++)
                fprintf(o, "%a ", S[v]);
        for (const int32_t *e : {p.edge_i, p.edge_j, p.edge_kind})
            for (int k = 0; k < p.n_edges; k++)
                fprintf(o, "%d ", e[k]);
        for (MapPoint *m : g.points)
            fprintf(o, "%d ", sc.mp_index(m));
        for (int m = 0; m < M; m++)
            fprintf(o, "%d ", g.point_ref[(size_t)m]);
        for (int m = 0; m < 3 * M; m++)
            fprintf(o, "%a ", (double)g.world_pos[(size_t)m]);
        fclose(o);
    } catch (const std::exception &e) {
        std::cerr << e.what() << "\n";
        return 1;
    }
    std::cout << "eg shim ok\n";
    return 0;
}
