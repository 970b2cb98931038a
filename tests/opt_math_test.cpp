// Host build of csrc/opt_math.h, the FP64 helpers the device optimisers share: reads the cases tests/test_opt_math.py
// writes (one per line: a name, then hex doubles) and prints every result as a line of hex doubles, which the Python
// side compares byte for byte with tests/pose_model.py.  Built with g++ -ffp-contract=off and the sanitizers.
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

template <int N> static bool cholesky_case(const std::vector<double> &a)
{
    constexpr int T = N * (N + 1) / 2;
    if (a.size() != 1 + T + N)
        return false;
    double Hu[T], b[N], x[N], out[1 + N];
    for (int k = 0; k < T; k++)
        Hu[k] = a[1 + k];
    for (int k = 0; k < N; k++) {
        b[k] = a[1 + T + k];
        x[k] = -1.0;  // the solve has to write every entry, refused or not
    }
    out[0] = cholesky_solve<N>(Hu, a[0], b, x) ? 1.0 : 0.0;
    for (int k = 0; k < N; k++)
        out[1 + k] = x[k];
    print(out, 1 + N);
    return true;
}

template <int N> static bool lambda_case(const std::vector<double> &a)
{
    constexpr int T = N * (N + 1) / 2;
    if (a.size() != T)
        return false;
    double Hu[T];
    for (int k = 0; k < T; k++)
        Hu[k] = a[k];
    const double lam = lm_initial_lambda<N>(Hu);
    print(&lam, 1);
    return true;
}

static bool run(const std::string &op, const std::vector<double> &a)
{
    double o[9];
    if (op == "quat_from_matrix" && a.size() == 9) {
        quat_from_matrix(a.data(), o);
        print(o, 4);
    } else if (op == "quat_normalize" && a.size() == 4) {
        for (int i = 0; i < 4; i++)
            o[i] = a[i];
        quat_normalize(o);
        print(o, 4);
    } else if (op == "quat_to_matrix" && a.size() == 4) {
        quat_to_matrix(a.data(), o);
        print(o, 9);
    } else if (op == "quat_mul" && a.size() == 8) {
        quat_mul(a.data(), a.data() + 4, o);
        print(o, 4);
    } else if (op == "unit_quat_from_floats" && (a.size() == 9 || a.size() == 12)) {
        float m[12];
        for (size_t i = 0; i < a.size(); i++)
            m[i] = (float)a[i];
        unit_quat_from_floats(m, (int)a.size() / 3, o);
        print(o, 4);
    } else if (op == "huber" && a.size() == 3) {  // the trailing use_kernel left at its default
        huber(a[0], a[1], a[2], o[0], o[1]);
        print(o, 2);
    } else if (op == "huber" && a.size() == 4) {
        huber(a[0], a[1], a[2], o[0], o[1], a[3] != 0.0);
        print(o, 2);
    } else if (op == "lm_trial" && a.size() == 5) {  // cur, tmp, scale, lam, nu -> accepted, lam, nu, rho, stop
        double lam = a[3], nu = a[4], rho = -7.0;
        bool stop = false;
        o[0] = lm_trial(a[0], a[1], a[2], lam, nu, rho, stop) ? 1.0 : 0.0;
        o[1] = lam, o[2] = nu, o[3] = rho, o[4] = stop ? 1.0 : 0.0;
        print(o, 5);
    } else if (op == "cholesky_solve6") {
        return cholesky_case<6>(a);
    } else if (op == "cholesky_solve7") {
        return cholesky_case<7>(a);
    } else if (op == "lm_initial_lambda6") {
        return lambda_case<6>(a);
    } else if (op == "lm_initial_lambda7") {
        return lambda_case<7>(a);
    } else {
        return false;
    }
    return true;
}

int main(int argc, char **argv)
{
    if (argc != 2) {
        fprintf(stderr, "usage: opt_math_test <cases>\n");
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
