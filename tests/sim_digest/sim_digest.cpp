// sim_digest.cpp -- CPU logic checker of k_digest and k_digest_final (TEST INFRASTRUCTURE).
//
// Runs digest_item and digest_final of h263-rs_amd/csrc/digest_kernel.inl lane by lane: every work item of the launch, its 64
// lanes one after the other in each phase, the LDS hand-off a plain struct, the atomics plain additions.  The table goes through
// digest_table, the host half of the library.  Built by tests/test_sim_digest.py with g++ -fsanitize=address,undefined into a
// temporary directory; never part of the product.
//
//   sim_digest --piece
//        prints DIGEST_PIECE
//   sim_digest <in> <out>
//   in : u64 buffer_bytes; u32 n_spans, n_digests, n_seeds, fill; u32 seeds[n_seeds]; h263mi_digest_span spans[n_spans];
//        fill 0: buffer_bytes of data follow; fill 1: the buffer is all 0xFF and nothing follows
//   out: per seed: u32 status (0 = digested, 1 = the table was refused), then n_digests digests
// The buffer is allocated at exactly buffer_bytes: ASan sees a read one byte outside.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../h263-rs_amd/csrc/digest_kernel.inl"

using namespace h263mi;

static bool read_all(FILE *f, void *p, size_t n) { return fread(p, 1, n, f) == n; }

int main(int argc, char **argv)
{
    if (argc == 2 && !strcmp(argv[1], "--piece")) {
        printf("%u\n", DIGEST_PIECE);
        return 0;
    }
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb");
    if (!in) return 2;
    uint64_t buffer_bytes = 0;
    uint32_t hd[4];
    if (!read_all(in, &buffer_bytes, 8) || !read_all(in, hd, sizeof hd)) return 2;
    const uint32_t n_spans = hd[0], n_digests = hd[1], n_seeds = hd[2], fill = hd[3];
    std::vector<uint32_t> seeds(n_seeds);
    std::vector<h263mi_digest_span> spans(n_spans);
    if (!read_all(in, seeds.data(), 4 * seeds.size()) || !read_all(in, spans.data(), sizeof(h263mi_digest_span) * spans.size())) return 2;
    // (malloc: exactly as large as the data, 16-byte aligned like device memory)
    uint8_t *buf = (uint8_t *)malloc(buffer_bytes ? buffer_bytes : 1);
    if (!buf) return 2;
    if (fill) memset(buf, 0xFF, buffer_bytes);
    else if (!read_all(in, buf, buffer_bytes)) return 2;
    fclose(in);

    FILE *out = fopen(argv[2], "wb");
    if (!out) return 2;
    static DigestLds lds;
    static DigestLane lanes[64];
    auto each = [&](auto f) {
        for (int l = 0; l < 64; l++) f(l, lanes[l]);
    };
    for (uint32_t seed : seeds) {
        std::vector<uint32_t> result(1 + (size_t)n_digests, 0u);
        const bool have_base = buffer_bytes != 0;
        if (!digest_table(spans.data(), n_spans, n_digests, buffer_bytes, have_base, seed, nullptr, nullptr, nullptr)) {
            result[0] = 1;
        } else {
            std::vector<DigestSpan> table(n_spans);
            std::vector<unsigned long long> acc(2 * (size_t)n_digests);
            DigestArgs a{};
            digest_table(spans.data(), n_spans, n_digests, buffer_bytes, have_base, seed, table.data(), acc.data(), &a.n_items);
            a.base = buf;
            a.spans = table.data();
            a.acc = acc.data();
            a.n_spans = n_spans;
            // the launch's waves, last to first: the accumulation does not depend on the order of arrival
            for (uint64_t item = a.n_items; item-- > 0;) {
                memset(&lds, 0xA5, sizeof lds);
                memset(lanes, 0x5A, sizeof lanes);
                digest_item(a, lds, item, each);
            }
            DigestFinalArgs f{};
            f.acc = acc.data();
            f.out = result.data() + 1;
            f.n_digests = n_digests;
            for (uint32_t k = 0; k < n_digests; k++) digest_final(f, k);
        }
        if (fwrite(result.data(), 4, result.size(), out) != result.size()) return 2;
    }
    fclose(out);
    free(buf);
    return 0;
}
