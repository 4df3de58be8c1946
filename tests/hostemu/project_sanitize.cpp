// A stand-alone program for the sanitizers (-fsanitize=address,undefined; built and run by tests/test_point_project.py): the whole call of
// project_emu.cpp -- count, list, solve -- on a crafted scene in R^2 and on a chain of boxes in R^8, every array on the heap and exactly
// as long as the call may write.  Exit status 0: the answers are the expected ones.
#include <cmath>
#include <cstdio>
#include <vector>
#include "project_emu.cpp"

static int run(int n, int P, const std::vector<int> &ptr, const std::vector<double> &A, const std::vector<double> &b, int Q, const std::vector<double> &points,
               const std::vector<double> &radius, int max_iter, std::vector<long long> &hit_ptr, std::vector<int> &region, std::vector<unsigned char> &cls,
               std::vector<double> &distance, std::vector<double> &nearest, std::vector<int> &status, std::vector<int> &iterations)
{
    hit_ptr.assign((size_t)Q + 1, 0);
    const long long T = project_emu_call(n, P, ptr.data(), A.data(), b.data(), Q, points.data(), radius.empty() ? nullptr : radius.data(), max_iter, hit_ptr.data(),
                                         nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, -1);
    if (T < 0) return 1;
    region.assign((size_t)T, 0); cls.assign((size_t)T, 0); distance.assign((size_t)T, 0); nearest.assign((size_t)T * n, 0); status.assign((size_t)T, 0);
    iterations.assign((size_t)T, 0);
    return project_emu_call(n, P, ptr.data(), A.data(), b.data(), Q, points.data(), radius.empty() ? nullptr : radius.data(), max_iter, hit_ptr.data(), region.data(),
                            cls.data(), distance.data(), nearest.data(), status.data(), iterations.data(), T) == T ? 0 : 1;
}

int main()
{
    std::vector<long long> hit_ptr;
    std::vector<int> region, status, iterations;
    std::vector<unsigned char> cls;
    std::vector<double> distance, nearest;
    int bad = 0;
    {   // the unit square, the wedge y <= 0.1 x, -y <= 0.1 x, x <= 1, and the square with its first row twice
        const std::vector<int> ptr{0, 4, 7, 12};
        const std::vector<double> A{1, 0, 0, 1, -1, 0, 0, -1, -0.1, 1, -0.1, -1, 1, 0, 1, 0, 0, 1, -1, 0, 0, -1, 1000, 0};
        const std::vector<double> b{1, 1, 0, 0, 0, 0, 1, 1, 1, 0, 0, 1000};
        const std::vector<double> points{0.5, 0.5, 1.5, 1.25, -1e-5, 0.0}, radius{0.0, INFINITY, 1.0};
        bad += run(2, 3, ptr, A, b, 3, points, radius, 100, hit_ptr, region, cls, distance, nearest, status, iterations);
        // point 0, radius 0: inside the square and the third region, 0.45 from the wedge (not listed); point 1: all three; point 2: all
        // three within 1.  Entries: 0 1 | 2 3 4 | 5 6 7
        bad += hit_ptr != std::vector<long long>{0, 2, 5, 8};
        for (size_t t = 0; t < status.size(); ++t) bad += status[t] != 0;
        if (!bad) {
            bad += !(cls[0] == 1 && distance[0] == 0.0 && nearest[0] == 0.5 && nearest[1] == 0.5 && iterations[0] == 0);
            bad += !(nearest[2 * 2] == 1.0 && nearest[2 * 2 + 1] == 1.0 && nearest[2 * 4] == 1.0 && nearest[2 * 4 + 1] == 1.0);
            bad += !(std::fabs(distance[6] - 1e-5) < 1e-18 && std::fabs(nearest[2 * 6]) < 1e-18 && std::fabs(nearest[2 * 6 + 1]) < 1e-18);
        }
        bad += run(2, 3, ptr, A, b, 3, points, radius, 0, hit_ptr, region, cls, distance, nearest, status, iterations);      // no step allowed
        for (size_t t = 0; t < status.size(); ++t) bad += status[t] != (cls[t] == 1 ? 0 : -1);
    }
    {   // 300 boxes [j, j + 1] x [0, 1]^7 in R^8 (two chunks) and two points: one beyond a corner of box 3, one far from everything
        const int n = 8, P = 300;
        std::vector<int> ptr(P + 1);
        std::vector<double> A((size_t)P * 2 * n * n, 0.0), b((size_t)P * 2 * n);
        for (int j = 0; j < P; ++j) {
            ptr[j + 1] = 2 * n * (j + 1);
            for (int k = 0; k < n; ++k) {
                A[((size_t)j * 2 * n + k) * n + k] = 1.0; b[(size_t)j * 2 * n + k] = k == 0 ? j + 1.0 : 1.0;
                A[((size_t)j * 2 * n + n + k) * n + k] = -1.0; b[(size_t)j * 2 * n + n + k] = k == 0 ? -(double)j : 0.0;
            }
        }
        std::vector<double> points(2 * n, 1.5);
        points[0] = 3.5;
        for (int k = 0; k < n; ++k) points[n + k] = -100.0;
        bad += run(n, P, ptr, A, b, 2, points, std::vector<double>{1.5, 10.0}, 100, hit_ptr, region, cls, distance, nearest, status, iterations);
        bad += !(hit_ptr[2] == hit_ptr[1] && hit_ptr[1] > 0);
        for (long long t = 0; t < hit_ptr[1]; ++t)
            if (region[(size_t)t] == 3) bad += !(status[(size_t)t] == 0 && std::fabs(distance[(size_t)t] - 0.5 * std::sqrt(7.0)) < 1e-14 && nearest[(size_t)t * n] == 3.5);
        bad += run(n, P, ptr, A, b, 2, points, std::vector<double>{}, 100, hit_ptr, region, cls, distance, nearest, status, iterations);      // +inf: every pair
        bad += hit_ptr[2] != 2LL * P;
    }
    std::printf("%s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
