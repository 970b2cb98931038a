// Host build of csrc/sim3_math.h, the Sim3 arithmetic the two Sim3 optimisers share: reads the cases
// tests/test_sim3_math.py writes (one per line: a name, then hex doubles) and prints every result as a line of hex doubles,
// which the Python side compares with tests/eg_model.py and tests/sim3opt_model.py.  Built with g++ -ffp-contract=off and
// the sanitizers.  sim3_update prints both forms: the 8-double states' result, then (qn, tn, sn) of the (q, t, s) form.
#include "sim3_math.h"

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

using namespace orbgpu;

static void print(const double *v, int n)
{
    for (int i = 0; i < n; i++)
        printf("%a%c", v[i], i + 1 < n ? ' ' : '\n');
}

static bool run(const std::string &op, const std::vector<double> &a)
{
    double o[16];
    const double *p = a.data();
    if (op == "sim3_mul" && a.size() == 16) {
        sim3_mul(p, p + 8, o);
        print(o, 8);
    } else if (op == "sim3_inv" && a.size() == 8) {
        sim3_inv(p, o);
        print(o, 8);
    } else if (op == "sim3_map" && a.size() == 11) {
        sim3_map(p, p + 8, o);
        print(o, 3);
    } else if (op == "lu_solve3" && a.size() == 12) {
        lu_solve3(p, p + 9, o);
        print(o, 3);
    } else if (op == "chi2_of" && a.size() == 7) {
        o[0] = chi2_of(p);
        print(o, 1);
    } else if (op == "sim3_log" && a.size() == 8) {
        sim3_log(p, o);
        print(o, 7);
    } else if (op == "sim3_edge_error" && a.size() == 24) {
        sim3_edge_error(p, p + 8, p + 16, o);
        print(o, 7);
    } else if (op == "sim3_update" && a.size() == 16) {  // S[8], x[7], fix_scale
        double S[8];
        load8(p, S);
        sim3_update(S, p + 8, a[15] != 0.0, o);
        sim3_update(S, S + 4, S[7], p + 8, a[15] != 0.0, o + 8, o + 12, o[15]);
        print(o, 16);
    } else {
        return false;
    }
    return true;
}

int main(int argc, char **argv)
{
    if (argc != 2) {
        fprintf(stderr, "usage: sim3_math_test <cases>\n");
        return 2;
    }
    std::ifstream in(argv[1]);
    std::string line;
    int n = 0;
    while (std::getline(in, line)) {
        std::istringstream ss(line);
        std::string op, tok;
        ss >> op;
        std::vector<double> a;
        while (ss >> tok)
            a.push_back(strtod(tok.c_str(), nullptr));  // hex floats, "nan" and "inf"
        if (!run(op, a)) {
            fprintf(stderr, "bad case %d: %s\n", n, line.c_str());
            return 1;
        }
        n++;
    }
    return n > 0 ? 0 : 1;
}
