// A stand-alone program for the sanitizers (-fsanitize=address,undefined; built and run by tests/test_segment_clip.py): the whole call of
// clip_emu.cpp -- count, list, chain -- on a crafted scene in R^2, on regions with rows of zeros or no rows, and on a run of boxes in R^8
// over three chunks, every array on the heap and exactly as long as the call may write.  Exit status 0: the answers are the expected ones.
#include <cmath>
#include <cstdio>
#include <vector>
#include "clip_emu.cpp"

struct Result {
    std::vector<long long> hit_ptr, chain_ptr;
    std::vector<int> region, status, chain;
    std::vector<unsigned char> cls;
    std::vector<double> t_in, t_out, reach;
};

static int run(int n, int P, const std::vector<int> &ptr, const std::vector<double> &A, const std::vector<double> &b, int Q, const std::vector<double> &from,
               const std::vector<double> &to, double tol, Result &r)
{
    r.hit_ptr.assign((size_t)Q + 1, 0);
    const long long T = clip_emu_call(n, P, ptr.data(), A.data(), b.data(), Q, from.data(), to.data(), tol, r.hit_ptr.data(), nullptr, nullptr, nullptr, nullptr,
                                      nullptr, nullptr, nullptr, nullptr, -1);
    if (T < 0) return 1;
    r.region.assign((size_t)T, 0); r.cls.assign((size_t)T, 0); r.t_in.assign((size_t)T, 0); r.t_out.assign((size_t)T, 0); r.chain.assign((size_t)T, 0);
    r.status.assign((size_t)Q, -7); r.reach.assign((size_t)Q, -7.0); r.chain_ptr.assign((size_t)Q + 1, -7);
    return clip_emu_call(n, P, ptr.data(), A.data(), b.data(), Q, from.data(), to.data(), tol, r.hit_ptr.data(), r.region.data(), r.cls.data(), r.t_in.data(),
                         r.t_out.data(), r.status.data(), r.reach.data(), r.chain_ptr.data(), r.chain.data(), T) == T ? 0 : 1;
}

// the box [lo, hi] in R^2 appended to (ptr, A, b)
static void box2(std::vector<int> &ptr, std::vector<double> &A, std::vector<double> &b, double x0, double y0, double x1, double y1)
{
    const double rows[] = {1, 0, 0, 1, -1, 0, 0, -1}, rhs[] = {x1, y1, -x0, -y0};
    A.insert(A.end(), rows, rows + 8); b.insert(b.end(), rhs, rhs + 4);
    ptr.push_back(ptr.back() + 4);
}

int main()
{
    Result r;
    int bad = 0;
    {   // [0, 1]^2, [1, 2] x [0, 1] (they only abut), [2 + 1e-6, 3] x [0, 1]; a row 0 x <= -1 beside 0 x <= 1; no row at all (listed last)
        std::vector<int> ptr{0};
        std::vector<double> A, b;
        box2(ptr, A, b, 0, 0, 1, 1); box2(ptr, A, b, 1, 0, 2, 1); box2(ptr, A, b, 2 + 1e-6, 0, 3, 1);
        A.insert(A.end(), {0, 0, 0, 0}); b.insert(b.end(), {-1, 1}); ptr.push_back(ptr.back() + 2);
        const std::vector<double> from{0.25, 0.5, 1.25, 0.5, 0.5, 0.5, 5, 5}, to{1.75, 0.5, 2.75, 0.5, 0.5, 0.5, 5, 5};
        bad += run(2, 4, ptr, A, b, 4, from, to, 1e-9, r);
        // covered through the inflation by the chain 0, 1; a gap where box 1 ends; a point in box 0; a point in nothing
        bad += r.hit_ptr != std::vector<long long>{0, 2, 4, 5, 5} || r.status != std::vector<int>{0, 1, 0, 1};
        bad += r.chain_ptr != std::vector<long long>{0, 2, 3, 4, 4} || r.chain != std::vector<int>{0, 1, 2, 4, 0};
        if (!bad) bad += !(r.reach[0] == 1.0 && std::fabs(r.reach[1] - (0.75 + 1e-9) / 1.5) < 1e-11 && r.reach[2] == 1.0 && r.reach[3] == 0.0 && r.cls[4] == 1);
        ptr.push_back(ptr.back());      // the region without rows: WHOLE for every segment, so everything is covered
        bad += run(2, 5, ptr, A, b, 4, from, to, 1e-9, r);
        bad += r.hit_ptr != std::vector<long long>{0, 3, 6, 8, 9} || r.status != std::vector<int>{0, 0, 0, 0};
        bad += run(2, 5, ptr, A, b, 0, {}, {}, 1e-9, r);      // no segment
        bad += r.hit_ptr != std::vector<long long>{0} || r.chain_ptr != std::vector<long long>{0};
    }
    {   // 600 boxes [j, j + 1.5] x [0, 1]^7 in R^8 (three chunks, a partial last) and two segments: along all of them, and short of the first
        const int n = 8, P = 600;
        std::vector<int> ptr(P + 1);
        std::vector<double> A((size_t)P * 2 * n * n, 0.0), b((size_t)P * 2 * n);
        for (int j = 0; j < P; ++j) {
            ptr[j + 1] = 2 * n * (j + 1);
            for (int k = 0; k < n; ++k) {
                A[((size_t)j * 2 * n + k) * n + k] = 1.0; b[(size_t)j * 2 * n + k] = k == 0 ? j + 1.5 : 1.0;
                A[((size_t)j * 2 * n + n + k) * n + k] = -1.0; b[(size_t)j * 2 * n + n + k] = k == 0 ? -(double)j : 0.0;
            }
        }
        std::vector<double> from(2 * n, 0.5), to(2 * n, 0.5);
        from[0] = 0.25; to[0] = P + 0.25; from[n] = -3.0; to[n] = -1.0;
        bad += run(n, P, ptr, A, b, 2, from, to, 1e-9, r);
        bad += r.hit_ptr != std::vector<long long>{0, P, P} || r.status != std::vector<int>{0, 1} || r.chain_ptr != std::vector<long long>{0, P, P};
        for (int j = 0; !bad && j < P; ++j) bad += r.chain[(size_t)j] != j;
    }
    std::printf("%s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
