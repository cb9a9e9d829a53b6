// Stand-alone host program over csrc/ensemble_clip_body.h (tests/ensemble_clip_checks.py builds it with the host compiler and
// -ffp-contract=off): the referee of nic_ensemble_adam_prepare_clipped / _update_clipped, bit for bit.
//   run IN OUT                      -> `steps` clipped Adam steps on the buffers of IN, the results to OUT (formats below)
//   check_prepare n_models P hyper max_norm state coef grads clip grads_stride          (pointers: 0 = null, else non-null)
//   check_update n_models P params grads exp_avg exp_avg_sq coef clip params_stride grads_stride exp_avg_stride exp_avg_sq_stride
//                                   -> refusal code and reason of the request checks
// IN : int64 K, P, steps, params_stride, grads_stride, exp_avg_stride, exp_avg_sq_stride; double hyper[K][5]; double max_norm[K];
//      NicEnsembleAdamState state[K]; float params[K][ps], grads[steps][K][gs], exp_avg[K][es], exp_avg_sq[K][vs]
// OUT: float params[K][ps], exp_avg[K][es], exp_avg_sq[K][vs]; NicEnsembleAdamState state[K]; float coef[K][8];
//      float clip[steps][K][2] ({scale, norm} of every step)
// Columns at or past P of a row are carried through untouched, whatever their bits, and never read.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../neural_inventory_control_amd/csrc/ensemble_clip_body.h"

static long long arg(char** v, int i) { return atoll(v[i]); }
static const void* fake(char** v, int i) { return arg(v, i) ? (const void*)v : nullptr; }

template <class T>
static bool rd(FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}
template <class T>
static bool wr(FILE* f, const std::vector<T>& v) { return v.empty() || fwrite(v.data(), sizeof(T), v.size(), f) == v.size(); }

static int run(const char* in, const char* out) {
    FILE* f = fopen(in, "rb");
    if (!f) return 3;
    int64_t h[7];
    if (fread(h, sizeof(int64_t), 7, f) != 7) return 3;
    const int64_t K = h[0], P = h[1], steps = h[2], ps = h[3], gs = h[4], es = h[5], vs = h[6];
    std::vector<double> hyper, max_norm;
    std::vector<NicEnsembleAdamState> state;
    std::vector<float> params, grads, exp_avg, exp_avg_sq, coef((size_t)K * nic::EA_COEF_COUNT, 0.f);
    if (K < 1 || steps < 0 || !rd(f, hyper, K * nic::EA_HYPER_COUNT) || !rd(f, max_norm, K) || !rd(f, state, K) || !rd(f, params, K * ps) ||
        !rd(f, grads, steps * K * gs) || !rd(f, exp_avg, K * es) || !rd(f, exp_avg_sq, K * vs))
        return 3;
    fclose(f);
    std::vector<float> clip((size_t)(steps * K) * nic::EC_CLIP_COUNT, 0.f);
    for (int64_t s = 0; s < steps; ++s) {
        const float* g = grads.data() + s * K * gs;
        float* cl = clip.data() + s * K * nic::EC_CLIP_COUNT;
        if (int r = nic::ec_check_prepare((int)K, (int)P, hyper.data(), max_norm.data(), state.data(), coef.data(), g, gs, cl)) return 10 + r;
        if (int r = nic::ec_check_update((int)K, (int)P, params.data(), ps, g, gs, exp_avg.data(), es, exp_avg_sq.data(), vs, coef.data(), cl))
            return 10 + r;
        for (int64_t m = 0; m < K; ++m)
            nic::ec_finish(nic::ec_row_sum(g + m * gs, (int)P), max_norm[m], &hyper[m * nic::EA_HYPER_COUNT], &state[m],
                           &coef[m * nic::EA_COEF_COUNT], cl + m * nic::EC_CLIP_COUNT);
        for (int64_t m = 0; m < K; ++m)
            for (int64_t c = 0; c < P; ++c)
                nic::ec_update(&params[m * ps + c], g[m * gs + c], cl[m * nic::EC_CLIP_COUNT + nic::EC_SCALE], &exp_avg[m * es + c],
                               &exp_avg_sq[m * vs + c], &coef[m * nic::EA_COEF_COUNT]);
    }
    f = fopen(out, "wb");
    if (!f || !wr(f, params) || !wr(f, exp_avg) || !wr(f, exp_avg_sq) || !wr(f, state) || !wr(f, coef) || !wr(f, clip)) return 4;
    fclose(f);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const char* what = argv[1];
    if (!strcmp(what, "run") && argc == 4) return run(argv[2], argv[3]);
    if (!strcmp(what, "check_prepare") && argc == 11) {
        const int r = nic::ec_check_prepare((int)arg(argv, 2), (int)arg(argv, 3), fake(argv, 4), fake(argv, 5), fake(argv, 6), fake(argv, 7),
                                            fake(argv, 8), arg(argv, 10), fake(argv, 9));
        printf("%d %s\n", r, nic::ea_reason(r));
        return 0;
    }
    if (!strcmp(what, "check_update") && argc == 14) {
        const int r = nic::ec_check_update((int)arg(argv, 2), (int)arg(argv, 3), fake(argv, 4), arg(argv, 10), fake(argv, 5), arg(argv, 11),
                                           fake(argv, 6), arg(argv, 12), fake(argv, 7), arg(argv, 13), fake(argv, 8), fake(argv, 9));
        printf("%d %s\n", r, nic::ea_reason(r));
        return 0;
    }
    fprintf(stderr, "ensemble_clip_harness: bad arguments\n");
    return 2;
}
