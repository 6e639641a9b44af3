// Stand-alone driver of the reference descriptors of a fidelity call
// (gsc_envelope.h: gsc::fidelity_refs), meant for a host sanitizer build:
//   make -C soundchunks_amd/csrc fidelity_check
// What the helper keeps (a pointer with a positive length, whatever its
// alignment), what it turns into a null reference (any pointer with 0
// samples), that it writes out[0 .. n) and nothing past it, and its refusals,
// each naming the first stream at fault: a negative length, a null pointer
// with a positive length, missing arrays.  No pointer is dereferenced: the
// references are device memory to the library.  Exit status 0 when nothing
// failed.
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../soundchunks_amd/csrc/gsc_envelope.h"

namespace {

int g_bad = 0;

#define CHECK(cond, ...)                                               \
    do {                                                               \
        if (!(cond)) {                                                 \
            std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); \
            std::printf(__VA_ARGS__);                                  \
            std::printf("\n");                                         \
            ++g_bad;                                                   \
            return;                                                    \
        }                                                              \
    } while (0)

// never read: stand-ins for device addresses, the second one 2-byte aligned only
int16_t g_store[8];

void check_good() {
    const void* a = g_store;
    const void* odd = g_store + 1;
    const std::vector<const void*> pcm = {a, nullptr, odd, a, odd};
    const std::vector<int64_t> samples = {100, 0, 1, 0, int64_t(1) << 40};
    const int n = int(pcm.size());
    // exactly n entries: the sanitizer sees a write past them
    std::vector<gsc::FidelityRef> out(static_cast<size_t>(n), gsc::FidelityRef{static_cast<const int16_t*>(a), -7});
    std::string err = "untouched";
    CHECK(gsc::fidelity_refs(pcm.data(), samples.data(), n, out.data(), &err) == 0, "refused: %s", err.c_str());
    CHECK(err == "untouched", "a good call wrote its error: %s", err.c_str());
    for (int i = 0; i < n; ++i) {
        const gsc::FidelityRef& r = out[size_t(i)];
        CHECK(r.samples == samples[size_t(i)], "stream %d: %lld samples", i, (long long)r.samples);
        const void* want = samples[size_t(i)] > 0 ? pcm[size_t(i)] : nullptr;
        CHECK(static_cast<const void*>(r.pcm) == want, "stream %d: pointer", i);
    }
    // no streams: nothing is read or written
    CHECK(gsc::fidelity_refs(nullptr, nullptr, 0, nullptr, &err) == 0, "n = 0 refused: %s", err.c_str());
    std::printf("kept, dropped to null and counted: ok (%d streams)\n", n);
}

void check_refusals() {
    const void* a = g_store;
    struct Case {
        std::vector<const void*> pcm;
        std::vector<int64_t> samples;
        const char* want;
    };
    const std::vector<Case> cases = {
        {{a, a}, {5, -1}, "stream 1: the reference has -1 samples"},
        {{a, nullptr}, {-3, -1}, "stream 0: the reference has -3 samples"},
        {{nullptr, a}, {0, INT64_MIN}, "stream 1: the reference has -9223372036854775808 samples"},
        {{a, nullptr, nullptr}, {5, 0, 2}, "stream 2: the reference is null and has 2 samples"},
        {{nullptr}, {1}, "stream 0: the reference is null and has 1 samples"},
    };
    for (const Case& c : cases) {
        const int n = int(c.pcm.size());
        std::vector<gsc::FidelityRef> out(static_cast<size_t>(n));
        std::string err;
        CHECK(gsc::fidelity_refs(c.pcm.data(), c.samples.data(), n, out.data(), &err) == -1, "%s: accepted", c.want);
        CHECK(err.find(c.want) != std::string::npos, "%s: got \"%s\"", c.want, err.c_str());
        // without a place for the message
        CHECK(gsc::fidelity_refs(c.pcm.data(), c.samples.data(), n, out.data(), nullptr) == -1, "%s: accepted", c.want);
    }
    const int64_t one = 1;
    gsc::FidelityRef r{};
    std::string err;
    CHECK(gsc::fidelity_refs(&a, &one, -1, &r, &err) == -1 && err == "gsc fidelity: invalid argument", "n = -1");
    CHECK(gsc::fidelity_refs(nullptr, &one, 1, &r, &err) == -1 && err == "gsc fidelity: invalid argument", "no pcm");
    CHECK(gsc::fidelity_refs(&a, nullptr, 1, &r, &err) == -1 && err == "gsc fidelity: invalid argument", "no samples");
    CHECK(gsc::fidelity_refs(&a, &one, 1, nullptr, &err) == -1 && err == "gsc fidelity: invalid argument", "no out");
    std::printf("refusals: ok (%zu cases, 4 invalid calls)\n", cases.size());
}

}  // namespace

int main() {
    check_good();
    check_refusals();
    if (g_bad) std::printf("%d check(s) failed\n", g_bad);
    return g_bad ? 1 : 0;
}
