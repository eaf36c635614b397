// Host-only check of the multiplier planner's split Karatsuba plans and of its table image
// (mul_plan.h), under ASan/UBSan: the planner header is compiled into this driver and nothing else
// is linked, no hm_ctx and no GPU.  Built and run by tests/test_sanitize.py.
//  - K = 16 with a 2^18-word scratch limit splits products into subtree programs, and the split
//    plan issues exactly the leaf products of the breadth-first plan (the same multiset of leaf
//    shapes), with every scratch region below the limit's bound;
//  - K = 21 plans with the default limit (its largest product needs 3.1e8 scratch words
//    breadth-first, past the 28-bit views), and K = 20's default plan is not split;
//  - pack_tables puts the K = 16 plan's 17 tables at 16-byte aligned offsets of the image, in
//    order and in range, each holding the bytes of the vector it came from.
#include "../../homomorph-rust_amd/csrc/mul_plan.h"

#include <cstdio>
#include <tuple>

static int fails = 0;
#define CHECK(c)                                                                                  \
    do {                                                                                          \
        if (!(c)) {                                                                               \
            std::fprintf(stderr, "FAIL %s:%d %s\n", __FILE__, __LINE__, #c);                      \
            ++fails;                                                                              \
        }                                                                                         \
    } while (0)

static bool plan(uint32_t K, uint64_t scratch, hm::MulPlan &P) {
    P.L = 32, P.K = K, P.is_signed = false;
    P.ab.assign(K, 256), P.bb.assign(K, 256);
    P.ka_min = 256, P.ka_leaf = 256, P.mfma = true, P.ka_scratch = scratch;
    return hm::build_plan(P);
}

static size_t subprograms(const hm::MulPlan &P) {
    size_t n = 0;
    for (const auto &c : P.cols)
        for (const auto &g : c.ka) n += !g.deg;
    return n;
}

static std::vector<std::tuple<uint32_t, uint32_t, uint32_t>> leaf_shapes(const hm::MulPlan &P) {
    std::vector<std::tuple<uint32_t, uint32_t, uint32_t>> v;
    for (const auto &t : P.ka_vtasks) v.emplace_back(t.nu, t.nv, t.nout);
    std::sort(v.begin(), v.end());
    return v;
}

// the image pack_tables makes of a plan's tables
static void check_image(hm::MulPlan &P) {
    const std::vector<uint8_t> img = hm::pack_tables(P);
    size_t ntables = 0, end = 0;
    hm::for_each_table(P, [&](size_t off, const auto &v) {
        const size_t n = hm::table_bytes(v);
        CHECK(off % 16 == 0 && off >= end && off + n <= img.size());
        CHECK(n == 0 || std::memcmp(img.data() + off, v.data(), n) == 0);
        end = off + n;
        ++ntables;
    });
    CHECK(ntables == 17);
    CHECK(img.size() % 16 == 0 && img.size() >= 16 && img.size() < end + 16);
    CHECK(P.off_slots == 0 && !P.slots.empty() && P.off_ka_combs > P.off_ka_vtiles);
}

int main() {
    hm::MulPlan whole, split;
    CHECK(plan(16, hm::kKaScratchWords, whole));
    CHECK(plan(16, 1u << 18, split));
    CHECK(subprograms(whole) == 0);
    CHECK(subprograms(split) > 0);
    CHECK(whole.ka_vtasks.size() == split.ka_vtasks.size());
    CHECK(leaf_shapes(whole) == leaf_shapes(split));
    CHECK(split.astride < whole.astride); // less scratch per value
    check_image(whole);
    check_image(split);
    hm::MulPlan k20, k21;
    CHECK(plan(20, hm::kKaScratchWords, k20));
    CHECK(subprograms(k20) == 0);
    CHECK(plan(21, hm::kKaScratchWords, k21));
    CHECK(subprograms(k21) > 0);
    if (fails) return 1;
    std::printf("ok (K = 16: %zu split programs, %zu leaves; K = 21: %zu split programs)\n",
                subprograms(split), split.ka_vtasks.size(), subprograms(k21));
    return 0;
}
