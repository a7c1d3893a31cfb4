// The host-only pieces of mi_knn_search_diverse (image_search_amd/csrc/diverse_host.h) as a stand-alone program: the argument
// rules, the record's layout and the copy into caller arrays of exactly k / pool elements, some of them absent.  Built with
// -fsanitize=address,undefined (tests/test_diverse_host.py) every array is heap memory of its exact size, so a write one
// element too far is reported.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../image_search_amd/csrc/diverse_host.h"

using namespace mi;

static int failures = 0;
#define EXPECT(x) do { if (!(x)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); ++failures; } } while (0)

static void args() {
    const char* why = nullptr;
    int t = 0, q = 0, o = 0;
    const uint64_t ids[1] = {0};
    EXPECT(diverse_check_args(&t, &q, 1, 1, 0.0f, nullptr, 0, &o, &o, &why) == MI_OK);
    EXPECT(diverse_check_args(&t, &q, 4096, 4096, INFINITY, ids, 1, &o, &o, &why) == MI_OK);
    EXPECT(diverse_check_args(&t, &q, 1, 64, 0.05f, ids, 0, &o, &o, &why) == MI_OK);
    EXPECT(diverse_check_args(nullptr, &q, 1, 1, 0.0f, nullptr, 0, &o, &o, &why) == MI_ERR_INVALID);
    EXPECT(diverse_check_args(&t, nullptr, 1, 1, 0.0f, nullptr, 0, &o, &o, &why) == MI_ERR_INVALID);
    EXPECT(diverse_check_args(&t, &q, 1, 1, 0.0f, nullptr, 0, nullptr, &o, &why) == MI_ERR_INVALID);
    EXPECT(diverse_check_args(&t, &q, 1, 1, 0.0f, nullptr, 0, &o, nullptr, &why) == MI_ERR_INVALID);
    EXPECT(diverse_check_args(&t, &q, 0, 1, 0.0f, nullptr, 0, &o, &o, &why) == MI_ERR_INVALID);
    EXPECT(diverse_check_args(&t, &q, 1, 0, 0.0f, nullptr, 0, &o, &o, &why) == MI_ERR_INVALID);
    EXPECT(diverse_check_args(&t, &q, 0, 5000, 0.0f, nullptr, 0, &o, &o, &why) == MI_ERR_INVALID);   // zero before "too large"
    EXPECT(diverse_check_args(&t, &q, 1, 1, NAN, nullptr, 0, &o, &o, &why) == MI_ERR_INVALID);
    EXPECT(diverse_check_args(&t, &q, 1, 1, -1e-9f, nullptr, 0, &o, &o, &why) == MI_ERR_INVALID);
    EXPECT(diverse_check_args(&t, &q, 1, 1, 0.0f, nullptr, 3, &o, &o, &why) == MI_ERR_INVALID);
    EXPECT(diverse_check_args(&t, &q, 1, 4097, 0.0f, nullptr, 0, &o, &o, &why) == MI_ERR_UNSUPPORTED);
    EXPECT(diverse_check_args(&t, &q, 65, 64, 0.0f, nullptr, 0, &o, &o, &why) == MI_ERR_UNSUPPORTED);
    EXPECT(why && why[0] != '\0');
}

static void record(uint32_t k, uint32_t pool, bool with_optional) {
    const DiverseRecord r = diverse_record(k, pool);
    EXPECT(r.idx == 0 && r.dist == 8ull * k && r.hidden == 12ull * k && r.rep == 16ull * k && r.state == 16ull * k + 4ull * pool);
    EXPECT(r.bytes == r.state + 16 && r.dist % 4 == 0 && r.rep % 4 == 0 && r.state % 4 == 0);
    std::vector<unsigned char> rec(r.bytes);
    for (uint32_t j = 0; j < k; ++j) {
        reinterpret_cast<uint64_t*>(rec.data() + r.idx)[j] = 1000 + j;
        reinterpret_cast<float*>(rec.data() + r.dist)[j] = 0.5f * (float)j;
        reinterpret_cast<uint32_t*>(rec.data() + r.hidden)[j] = 7 * j;
    }
    for (uint32_t p = 0; p < pool; ++p) reinterpret_cast<uint32_t*>(rec.data() + r.rep)[p] = p % k;
    const uint32_t st[4] = {k, 3, 5, pool};
    for (int i = 0; i < 4; ++i) reinterpret_cast<uint32_t*>(rec.data() + r.state)[i] = st[i];

    // heap arrays of exactly the contract's sizes
    uint64_t* idx = new uint64_t[k];
    float* dist = new float[k];
    uint32_t* hidden = with_optional ? new uint32_t[k] : nullptr;
    uint32_t* rep = with_optional ? new uint32_t[pool] : nullptr;
    uint32_t* n_kept = with_optional ? new uint32_t[1] : nullptr;
    uint32_t state[4] = {0, 0, 0, 0};
    diverse_unpack(rec.data(), k, pool, idx, dist, hidden, rep, n_kept, state);
    for (uint32_t j = 0; j < k; ++j) {
        EXPECT(idx[j] == 1000 + j && dist[j] == 0.5f * (float)j);
        if (hidden) EXPECT(hidden[j] == 7 * j);
    }
    if (rep)
        for (uint32_t p = 0; p < pool; ++p) EXPECT(rep[p] == p % k);
    if (n_kept) EXPECT(*n_kept == k);
    for (int i = 0; i < 4; ++i) EXPECT(state[i] == st[i]);

    diverse_pad(k, pool, idx, dist, hidden, rep, n_kept);
    for (uint32_t j = 0; j < k; ++j) {
        EXPECT(idx[j] == MI_KNN_NO_ID && std::isinf(dist[j]) && dist[j] > 0);
        if (hidden) EXPECT(hidden[j] == 0);
    }
    if (rep)
        for (uint32_t p = 0; p < pool; ++p) EXPECT(rep[p] == MI_KNN_NO_LABEL);
    if (n_kept) EXPECT(*n_kept == 0);
    delete[] idx; delete[] dist; delete[] hidden; delete[] rep; delete[] n_kept;
}

int main() {
    args();
    for (const bool opt : {true, false}) {
        record(1, 1, opt);
        record(1, 64, opt);
        record(3, 7, opt);
        record(130, 130, opt);
        record(2304, 4096, opt);
        record(4096, 4096, opt);
    }
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("ok\n");
    return 0;
}
