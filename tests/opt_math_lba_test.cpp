// Host build of what csrc/opt_math.h holds for the local bundle adjustment (inv3_sym, point_update, llt_solve): reads the
// cases tests/test_opt_math_lba.py writes (one per line: a name, then hex doubles) and prints every result as a line of hex
// doubles, which the Python side compares byte for byte with tests/lba_model.py.  Built with g++ -ffp-contract=off and the
// sanitizers, like tests/opt_math_test.cpp.
#include "opt_math.h"

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
    double o[9];
    if (op == "inv3_sym" && a.size() == 7) {
        inv3_sym(a.data(), a[6], o);
        print(o, 9);
    } else if (op == "point_update" && a.size() == 6) {
        point_update(a.data(), a.data() + 3, o);
        print(o, 3);
    } else if (op == "llt_solve" && !a.empty()) {  // n, the packed lower triangle, b
        const int n = (int)a[0];
        const size_t tri = tri_at(n, 0);
        if (n < 0 || a.size() != 1 + tri + (size_t)n)
            return false;
        std::vector<double> A(a.begin() + 1, a.begin() + 1 + tri), v(a.begin() + 1 + tri, a.end()), work(2 * (size_t)n + 1);
        std::vector<double> out(1 + (size_t)n);
        out[0] = llt_solve(n, A.data(), v.data(), work.data(), 0, 1, NoBarrier()) ? 1.0 : 0.0;
        for (int i = 0; i < n; i++)
            out[1 + i] = v[i];
        print(out.data(), 1 + n);
    } else {
        return false;
    }
    return true;
}

int main(int argc, char **argv)
{
    if (argc != 2) {
        fprintf(stderr, "usage: opt_math_lba_test <cases>\n");
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
            a.push_back(strtod(tok.c_str(), nullptr));  // hex floats and "nan"
        if (!run(op, a)) {
            fprintf(stderr, "bad case %d: %s\n", n, line.c_str());
            return 1;
        }
        n++;
    }
    return n > 0 ? 0 : 1;
}
