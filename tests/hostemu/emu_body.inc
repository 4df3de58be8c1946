// body of one emulator instantiation (included by emu.cpp inside a namespace that pulls in one vertex_program namespace,
// with EMU_NAME = the exported function)


template <int N> struct CpuExec {
    Lane<N> Ls[WAVE];
    std::vector<int> solve_iters;      // count() of this wavefront's vertices, in lane order = slot order
    template <class F> void each(F &&f) { for (int l = 0; l < WAVE; ++l) f(Ls[l], l); }
    template <class P> bool all(P &&p) { for (int l = 0; l < WAVE; ++l) if (!p(Ls[l])) return false; return true; }
    void count(int *c, int fails, int iters) { c[0] += fails; c[1] += iters; solve_iters.push_back(iters); }
    void note(int *p, int v) { *p = v; }
    template <class F> int wave_max(F &&f) { int m = 0; for (int l = 0; l < WAVE; ++l) m = std::max(m, f(Ls[l])); return m; }
    // lanes run in increasing order inside a phase: the head lane of a segment initialises the sum, the
    // following lanes of the segment accumulate (the GPU does the same reduction as a shuffle tree)
    template <int CNT> void seg_reduce(Lane<N> &L, double (&v)[CNT], double *sin, double *sout, int special, int op,
                                       bool contributes, int, bool)
    {
        if (!contributes) return;
        double *dst = L.out ? sout : sin;
        for (int k = 0; k < CNT; ++k) {
            if (L.seg_head) dst[k] = v[k];
            else if (k == special && op == 1) dst[k] = fmin(dst[k], v[k]);
            else if (k == special && op == 2) dst[k] = fmax(dst[k], v[k]);
            else dst[k] += v[k];
        }
    }
};

// warm-start records for the following steps of this instantiation (warm_start.h): warm + warm_ptr[v]; null = cold solves
static double *g_warm = nullptr;
static const long long *g_warm_ptr = nullptr;
#define EMU_CAT_(a, b) a##b
#define EMU_CAT(a, b) EMU_CAT_(a, b)
extern "C" void EMU_CAT(EMU_NAME, _set_warm)(double *warm, const long long *warm_ptr) { g_warm = warm; g_warm_ptr = warm_ptr; }
// Newton iterations of every generic vertex of the following steps ([V]; null = not recorded)
static int *g_iters = nullptr;
extern "C" void EMU_CAT(EMU_NAME, _set_iters)(int *iters) { g_iters = iters; }

// T: the state type of zedge, mu and copy (the handle's dtype on the device); everything else is double either way
template <class T>
static int emu_run(int n, int V, int E, int NI, const int *inc_ptr, const int *inc_edge, const int *inc_out,
                   const int *poly_ptr, const double *poly_A, const double *poly_b, const double *center,
                   int src, int dst, const T *zedge, const T *mu, double rho, double mu_scale,
                   double eps_edge, double ipm_tol, int ipm_max_iter, T *copy, double *xv, double *zv,
                   double *yv, int *counters, int *is_generic)
{
    if (n != 2 && n != 3 && n != 6) return 1;
    std::vector<int> deg_in(V, 0);
    int MM = 1;
    for (int v = 0; v < V; ++v) {
        for (int k = inc_ptr[v]; k < inc_ptr[v + 1]; ++k) deg_in[v] += !inc_out[k];
        MM = std::max(MM, poly_ptr[v + 1] - poly_ptr[v]);
    }
    std::vector<double> bc(poly_ptr[V]);
    for (int v = 0; v < V; ++v)
        for (int j = poly_ptr[v]; j < poly_ptr[v + 1]; ++j) {
            double s = poly_b[j];
            for (int k = 0; k < n; ++k) s -= poly_A[(size_t)j * n + k] * center[(size_t)v * n + k];
            bc[j] = s;
        }
    std::vector<int> wave_slot_ptr{0}, wave_vtx;
    const int align_rows = getenv("GCS_EMU_ALIGN") ? atoi(getenv("GCS_EMU_ALIGN")) : 1;   // exercise the aligned placement by default
    const int STORE_DL = getenv("GCS_EMU_STORE_DL") ? atoi(getenv("GCS_EMU_STORE_DL")) : 1;   // and the stored dual directions
    int lanes = 0, slots = 0;
    for (int v = 0; v < V; ++v) {
        const int d = inc_ptr[v + 1] - inc_ptr[v], din = deg_in[v];
        is_generic[v] = !(v == src || v == dst || din == 0 || d - din == 0);
        if (!is_generic[v]) continue;
        if (d + 1 > WAVE) return 2;
        int b = group_base(lanes, d, din, align_rows);
        if (b < 0 || slots + 1 > MAX_SLOTS) { wave_slot_ptr.push_back((int)wave_vtx.size()); slots = 0; b = group_base(0, d, din, align_rows); }
        wave_vtx.push_back(v); lanes = b + d + 1; slots += 1;
    }
    if ((int)wave_vtx.size() > wave_slot_ptr.back()) wave_slot_ptr.push_back((int)wave_vtx.size());
    const int n_waves = (int)wave_slot_ptr.size() - 1;
    VertexArgs<T> a;
    a.n_waves = n_waves; a.wave_slot_ptr = wave_slot_ptr.data(); a.wave_vtx = wave_vtx.data(); a.align_rows = align_rows; a.MM = MM;
    gcsadmm_k::StepArgs<T> &s = a;     // the inputs every vertex-step program shares (step_args.h)
    s.inc_ptr = inc_ptr; s.deg_in = deg_in.data(); s.inc_edge = inc_edge; s.poly_ptr = poly_ptr;
    s.poly_A = poly_A; s.poly_bc = bc.data(); s.center = center; s.E = E; s.NI = NI;
    s.zedge = zedge; s.mu = mu; s.copy = copy; s.xv = xv; s.zv = zv; s.yv = yv; s.counters = counters;
    s.eps_edge = eps_edge; s.ipm_tol = ipm_tol; s.ipm_max_iter = ipm_max_iter; s.warm = g_warm; s.warm_ptr = g_warm_ptr;
    std::vector<double> smem(lds_doubles(n, MM, MAX_SLOTS, STORE_DL));
    auto run_all = [&](auto *ex, auto ntag) {
        constexpr int NN = decltype(ntag)::value;
        for (int w = 0; w < n_waves; ++w) {
            std::fill(smem.begin(), smem.end(), 0.0 / 0.0);   // poison: reads of unwritten LDS show up as NaN
            WaveShared S;
            wave_shared_init(S, smem.data(), n, MM, STORE_DL);
            ex->solve_iters.clear();
            if (STORE_DL) run_vertex_program<NN, T, 1>(*ex, w, a, S, rho, mu_scale);
            else run_vertex_program<NN, T, 0>(*ex, w, a, S, rho, mu_scale);
            if (g_iters && (int)ex->solve_iters.size() == wave_slot_ptr[w + 1] - wave_slot_ptr[w])
                for (int k = 0; k < (int)ex->solve_iters.size(); ++k) g_iters[wave_vtx[wave_slot_ptr[w] + k]] = ex->solve_iters[k];
            else if (g_iters)
                for (int k = wave_slot_ptr[w]; k < wave_slot_ptr[w + 1]; ++k) g_iters[wave_vtx[k]] = -1;     // (not one count per vertex)
        }
        delete ex;
    };
    if (n == 2) run_all(new CpuExec<2>(), std::integral_constant<int, 2>());
    else if (n == 3) run_all(new CpuExec<3>(), std::integral_constant<int, 3>());
    else run_all(new CpuExec<6>(), std::integral_constant<int, 6>());
    return 0;
}

#define EMU_STEP_ARGS(T)                                                                                                        \
    int n, int V, int E, int NI, const int *inc_ptr, const int *inc_edge, const int *inc_out, const int *poly_ptr,              \
    const double *poly_A, const double *poly_b, const double *center, int src, int dst, const T *zedge, const T *mu,            \
    double rho, double mu_scale, double eps_edge, double ipm_tol, int ipm_max_iter, T *copy, double *xv, double *zv,            \
    double *yv, int *counters, int *is_generic
#define EMU_STEP_PASS                                                                                                           \
    n, V, E, NI, inc_ptr, inc_edge, inc_out, poly_ptr, poly_A, poly_b, center, src, dst, zedge, mu, rho, mu_scale, eps_edge,    \
    ipm_tol, ipm_max_iter, copy, xv, zv, yv, counters, is_generic
extern "C" int EMU_NAME(EMU_STEP_ARGS(double)) { return emu_run<double>(EMU_STEP_PASS); }
// f32 state: float zedge / mu in, a float copy out (the program's float instantiation: the S10k configuration of the device)
extern "C" int EMU_CAT(EMU_NAME, _f32)(EMU_STEP_ARGS(float)) { return emu_run<float>(EMU_STEP_PASS); }
#undef EMU_STEP_ARGS
#undef EMU_STEP_PASS
