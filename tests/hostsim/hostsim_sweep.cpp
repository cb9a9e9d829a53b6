// TEST INFRASTRUCTURE: the sweep chain of closed_form_body.h (KC candidate level vectors per lane) on the host, looping over
// chains and candidate groups the way closed_form_sweep_kernel's grid does.  Never linked into the product library.
#include "../../neural_inventory_control_amd/csrc/closed_form_body.h"

template <int NP, int MF, bool CHAIN, int KC>
static void sweep_all(const NicClosedFormDesc& d, const float* levels, int K, float* chain_totals, double* g_levels) {
    for (int k0 = 0; k0 < K; k0 += KC)
        for (int s = 0; s < d.S; ++s)
            for (int64_t b = 0; b < d.n_scenarios; ++b) {
                float g[KC][NP > 0 ? NP : 1] = {};
                float sums[KC][2] = {};
                nic::closed_form_sweep_chain<NP, MF, CHAIN, 0, KC>(d, levels, K, k0, chain_totals, s, b, g, sums);
                for (int i = 0; i < KC && k0 + i < K; ++i)
                    for (int j = 0; j < NP; ++j) g_levels[(k0 + i) * NP + j] += g[i][j];
            }
}

template <int KC>
static void sweep_kc(const NicClosedFormDesc& d, const float* levels, int K, float* chain_totals, double* g_levels) {
    const int np = g_levels ? d.n_levels : 0;
    if (d.policy == NIC_CF_ECHELON) {   // (slot counts as in hostsim_closed_form_rollout)
        switch (np) {
            case 0: sweep_all<0, NIC_MAX_SLOTS, true, KC>(d, levels, K, chain_totals, g_levels); break;
            case 3: sweep_all<3, NIC_MAX_SLOTS, true, KC>(d, levels, K, chain_totals, g_levels); break;
            case 4: sweep_all<4, NIC_MAX_SLOTS, true, KC>(d, levels, K, chain_totals, g_levels); break;
            default: sweep_all<5, NIC_MAX_SLOTS, true, KC>(d, levels, K, chain_totals, g_levels); break;
        }
    } else if (d.Ws <= 4) {
        if (np == 0) sweep_all<0, 4, false, KC>(d, levels, K, chain_totals, g_levels);
        else if (np == 1) sweep_all<1, 4, false, KC>(d, levels, K, chain_totals, g_levels);
        else sweep_all<2, 4, false, KC>(d, levels, K, chain_totals, g_levels);
    } else {
        if (np == 0) sweep_all<0, NIC_MAX_SLOTS, false, KC>(d, levels, K, chain_totals, g_levels);
        else if (np == 1) sweep_all<1, NIC_MAX_SLOTS, false, KC>(d, levels, K, chain_totals, g_levels);
        else sweep_all<2, NIC_MAX_SLOTS, false, KC>(d, levels, K, chain_totals, g_levels);
    }
}

extern "C" {
// levels [K][n_levels] (host); chain_totals [K][2][S][ldb]; g_levels: [K][n_levels] doubles (per candidate, the sum over all
// chains of d total / d level_j, added in hostsim_closed_form_rollout's order), or NULL for a forward-only run.  kc: 1, 2 or 4.
int hostsim_closed_form_sweep(const NicClosedFormDesc* d, const float* levels, int n_candidates, int kc, float* chain_totals,
                              double* g_levels) {
    if (kc == 1) sweep_kc<1>(*d, levels, n_candidates, chain_totals, g_levels);
    else if (kc == 2) sweep_kc<2>(*d, levels, n_candidates, chain_totals, g_levels);
    else if (kc == 4) sweep_kc<4>(*d, levels, n_candidates, chain_totals, g_levels);
    else return 1;
    return 0;
}
}
