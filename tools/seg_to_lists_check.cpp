// Stand-alone host check of yrss_seg_to_lists (yastack_amd/csrc/yrss_seg.cpp),
// meant for a sanitizer build on the CPU; no GPU, no Python:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all
//       -I include tools/seg_to_lists_check.cpp yastack_amd/csrc/yrss_seg.cpp
//       -o seg_to_lists_check && ./seg_to_lists_check
// Every array is heap-allocated at exactly the size the contract states, so a
// read or write past it is an AddressSanitizer report.  Valid inputs (random
// queues, every n around the segment size) must give the lists a direct stable
// compaction gives; corrupted ones (each offset and index value in turn, then
// random bytes) must give -EINVAL or, where the arrays stay consistent, lists
// that are a permutation inside bounds.
#include <errno.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <vector>

#include "yrss.h"

namespace {

uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint32_t rnd()
{
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return (uint32_t)(g_rng >> 32);
}

struct Case {
    uint32_t n, nbk, nseg;
    std::unique_ptr<uint8_t[]> idx;      // exactly n bytes
    std::unique_ptr<uint16_t[]> off;     // exactly nseg * (nbk + 1)
    std::vector<uint32_t> want_idx, want_start;
};

Case make(uint32_t n, uint32_t nbk)
{
    Case c;
    c.n = n;
    c.nbk = nbk;
    c.nseg = (n + YRSS_SEG_PKTS - 1) / YRSS_SEG_PKTS;
    c.idx.reset(new uint8_t[n ? n : 1]);
    c.off.reset(new uint16_t[c.nseg ? c.nseg * (nbk + 1) : 1]);
    std::vector<uint32_t> b(n);
    for (auto &x : b)
        x = rnd() % nbk;
    c.want_start.assign(nbk + 1, 0);
    for (uint32_t k = 0; k < nbk; ++k) {
        c.want_start[k] = (uint32_t)c.want_idx.size();
        for (uint32_t i = 0; i < n; ++i)
            if (b[i] == k)
                c.want_idx.push_back(i);
    }
    c.want_start[nbk] = n;
    for (uint32_t s = 0; s < c.nseg; ++s) {
        const uint32_t lo = s * YRSS_SEG_PKTS, hi = lo + YRSS_SEG_PKTS < n ? lo + YRSS_SEG_PKTS : n;
        uint32_t w = 0;
        for (uint32_t k = 0; k < nbk; ++k) {
            c.off[s * (nbk + 1) + k] = (uint16_t)w;
            for (uint32_t i = lo; i < hi; ++i)
                if (b[i] == k)
                    c.idx[lo + w++] = (uint8_t)(i - lo);
        }
        c.off[s * (nbk + 1) + nbk] = (uint16_t)w;
    }
    return c;
}

int run(const Case &c, std::vector<uint32_t> *qi, std::vector<uint32_t> *qs)
{
    // outputs at their exact sizes too
    std::unique_ptr<uint32_t[]> oi(new uint32_t[c.n ? c.n : 1]);
    std::unique_ptr<uint32_t[]> os(new uint32_t[c.nbk + 1]);
    const int rc = yrss_seg_to_lists(c.idx.get(), c.off.get(), c.n, c.nbk, oi.get(), os.get());
    if (rc == 0 && qi) {
        qi->assign(oi.get(), oi.get() + c.n);
        qs->assign(os.get(), os.get() + c.nbk + 1);
    }
    return rc;
}

int fail(const char *what, uint32_t n, uint32_t nbk, long a = 0, long b = 0)
{
    fprintf(stderr, "FAIL %s (n %u, nbk %u, %ld, %ld)\n", what, n, nbk, a, b);
    return 1;
}

}  // namespace

int main()
{
    const uint32_t sizes[] = {0, 1, 2, 255, 256, 257, 511, 512, 513, 4097};
    const uint32_t nbks[] = {1, 2, 4, 16, 257};
    unsigned valid = 0, refused = 0, consistent = 0;
    for (uint32_t n : sizes)
        for (uint32_t nbk : nbks) {
            Case c = make(n, nbk);
            std::vector<uint32_t> qi, qs;
            if (run(c, &qi, &qs) != 0 || qi != c.want_idx || qs != c.want_start)
                return fail("valid input", n, nbk);
            ++valid;
            if (n == 0 || n > 600 || nbk == 257)
                continue;
            // every offset word, set to each of a few values
            const uint16_t vals[] = {0, 1, 255, 256, 257, 0x7fff, 0xffff};
            for (uint32_t k = 0; k < c.nseg * (nbk + 1); ++k)
                for (uint16_t v : vals) {
                    const uint16_t keep = c.off[k];
                    if (v == keep)
                        continue;
                    c.off[k] = v;
                    const int rc = run(c, nullptr, nullptr);
                    // a moved inner boundary can still be a well-formed row
                    const bool edge = k % (nbk + 1) == 0 || k % (nbk + 1) == nbk;
                    if (rc != -EINVAL && (rc != 0 || edge))
                        return fail("offset", n, nbk, k, v);
                    rc ? ++refused : ++consistent;
                    c.off[k] = keep;
                }
            // every index byte, set past its segment
            for (uint32_t i = 0; i < n; ++i) {
                const uint32_t s = i / YRSS_SEG_PKTS;
                const uint32_t len = n - s * YRSS_SEG_PKTS < YRSS_SEG_PKTS ? n - s * YRSS_SEG_PKTS
                                                                           : (uint32_t)YRSS_SEG_PKTS;
                if (len == YRSS_SEG_PKTS)
                    continue;   // a byte cannot exceed a full segment
                const uint8_t keep = c.idx[i];
                for (uint32_t v : {len, 255u}) {
                    c.idx[i] = (uint8_t)v;
                    if (run(c, nullptr, nullptr) != -EINVAL)
                        return fail("index", n, nbk, i, v);
                    ++refused;
                }
                c.idx[i] = keep;
            }
            // random bytes everywhere
            for (int t = 0; t < 200; ++t) {
                Case r = make(n, nbk);
                for (uint32_t k = 0; k < r.nseg * (nbk + 1); ++k)
                    if (rnd() % 4 == 0)
                        r.off[k] = (uint16_t)(rnd() % 300);
                for (uint32_t i = 0; i < n; ++i)
                    if (rnd() % 8 == 0)
                        r.idx[i] = (uint8_t)rnd();
                const int rc = run(r, nullptr, nullptr);
                if (rc != 0 && rc != -EINVAL)
                    return fail("random", n, nbk, rc);
                rc ? ++refused : ++consistent;
            }
        }
    // null pointers and bucket counts out of range
    uint32_t one[2] = {0, 0};
    if (yrss_seg_to_lists(nullptr, nullptr, 1, 1, one, one) != -EINVAL ||
        yrss_seg_to_lists(nullptr, nullptr, 0, 0, one, one) != -EINVAL ||
        yrss_seg_to_lists(nullptr, nullptr, 0, YRSS_MAX_QUEUES + 2, one, one) != -EINVAL ||
        yrss_seg_to_lists(nullptr, nullptr, 0, 1, nullptr, nullptr) != -EINVAL ||
        yrss_seg_to_lists(nullptr, nullptr, 0, 1, nullptr, one) != 0)
        return fail("arguments", 0, 0);
    printf("seg_to_lists_check ok: %u valid, %u refused (-EINVAL), %u corrupted but well-formed\n",
           valid, refused, consistent);
    return 0;
}
