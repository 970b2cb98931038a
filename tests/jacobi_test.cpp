// Host build of the per-lane half of csrc/jacobi.h: reads the matrices tests/test_jacobi.py writes (one 4 x 4 per line, 16
// hex doubles in row order) and prints, per matrix, one line of bit patterns: jacobi4_lane<16> (the diagonal of A, then V in
// row order), jacobi4_lane<30> (the same), and null_vector4 of the matrix rounded to float.  The Python side compares every
// pattern with tests/jacobi_model.py / tests/newpts_model.py.  Built with g++ -ffp-contract=off and the sanitizers.
#include "jacobi.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

using namespace orbgpu;

static void print_bits(double v)
{
    uint64_t u;
    memcpy(&u, &v, sizeof u);
    printf("%016llx ", (unsigned long long)u);
}

template <int SWEEPS> static void jacobi_case(const std::vector<double> &a)
{
    double A[4][4], V[4][4];
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) {
            A[i][j] = a[4 * i + j];
            V[i][j] = -1.0;  // the solver has to write every entry
        }
    jacobi4_lane<SWEEPS>(A, V);
    for (int i = 0; i < 4; i++)
        print_bits(A[i][i]);
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++)
            print_bits(V[i][j]);
}

int main(int argc, char **argv)
{
    if (argc != 2) {
        fprintf(stderr, "usage: jacobi_test <matrices>\n");
        return 2;
    }
    std::ifstream in(argv[1]);
    std::string line;
    int n = 0;
    while (std::getline(in, line)) {
        std::istringstream ss(line);
        std::string tok;
        std::vector<double> a;
        while (ss >> tok)
            a.push_back(strtod(tok.c_str(), nullptr));  // hex floats, "nan" and "inf"
        if (a.size() != 16) {
            fprintf(stderr, "bad matrix %d: %s\n", n, line.c_str());
            return 1;
        }
        jacobi_case<16>(a);
        jacobi_case<30>(a);
        float Af[4][4], x4[4] = {-1.f, -1.f, -1.f, -1.f};
        for (int i = 0; i < 4; i++)
            for (int j = 0; j < 4; j++)
                Af[i][j] = (float)a[4 * i + j];
        null_vector4(Af, x4);
        for (int i = 0; i < 4; i++)
            print_bits((double)x4[i]);
        printf("\n");
        n++;
    }
    return n > 0 ? 0 : 1;
}
