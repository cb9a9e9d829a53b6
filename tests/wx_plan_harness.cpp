// Host build of the forward / input-gradient launch plan (csrc/wx_plan.h) for tests/test_wx_plan_host.py: compiled with the host
// compiler into a small shared library and called through ctypes on arrays of cases.
#include <stddef.h>

#include "../neural_inventory_control_amd/csrc/wx_plan.h"

extern "C" {

// in: n x {M, K, ncols, operands eligible, compute units, forced stream, forced tile} (-1: not forced)
// out: n x {kernel, grid; then the kernel's line of kWxGeometry: family, block rows, block columns, threads}
void nic_test_wx_plans(const int32_t* in, int32_t* out, size_t n) {
    for (size_t i = 0; i < n; ++i) {
        const int32_t* c = in + 7 * i;
        const nic::WxPlan p = nic::wx_plan(c[0], c[1], c[2], c[3] != 0, c[4], nic::WxForce{c[5], c[6]});
        const nic::WxGeometry& g = nic::kWxGeometry[p.kernel];
        const int32_t row[6] = {p.kernel, p.grid, g.family, g.bm, g.bn, g.threads};
        for (int j = 0; j < 6; ++j) out[6 * i + j] = row[j];
    }
}

// the same plan with the default WxForce argument
int nic_test_wx_plan_unforced(int M, int K, int ncols, int operands_ok, int cus) { return nic::wx_plan(M, K, ncols, operands_ok != 0, cus).kernel; }

int nic_test_wx_product_end() { return nic::WX_PRODUCT_END; }
int nic_test_wx_kernel_end() { return nic::WX_KERNEL_END; }

const char* nic_test_wx_kernel_name(int kernel, const char* epi) {
    static char name[64];
    nic::wx_kernel_name(name, sizeof(name), static_cast<nic::WxKernel>(kernel), epi);
    return name;
}

int nic_test_wx_operands(uint64_t ab_address, int64_t lda, int64_t ldb, int M, int K) { return nic::wx_operands(ab_address, lda, ldb, M, K) ? 1 : 0; }

// out: {MT = NT of bf16_wx_kernel, grid}
void nic_test_bf16_wx_tile(int M, int ncols, int cus, int64_t* out) {
    const nic::Bf16WxTile t = nic::bf16_wx_tile(M, ncols, cus);
    out[0] = t.mt_nt;
    out[1] = t.grid;
}
}
