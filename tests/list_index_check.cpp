// Host check of csrc/list_index.hpp (built and run by tests/test_list_index.py with the host
// compiler's address and undefined-behaviour sanitizers): random chunk counts with long runs of
// chunks without ids and full chunks of 1,024 ids, records that begin and end anywhere; every id
// of every record must be found, through the record's bracket, where a brute-force walk of the
// chunks puts it.
#include "list_index.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace sdl;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {  // xorshift64*
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return (uint32_t)((rng_state * 0x2545F4914F6CDD1Dull) >> 32);
}
static uint32_t below(uint32_t n) { return rnd() % n; }

static int failures = 0;
#define CHECK(c, ...)                                   \
    do {                                                \
        if (!(c)) {                                     \
            if (++failures <= 10) {                     \
                fprintf(stderr, "FAIL %s: ", #c);       \
                fprintf(stderr, __VA_ARGS__);           \
                fprintf(stderr, "\n");                  \
            }                                           \
        }                                               \
    } while (0)

// One arena of n chunks.  A piece is a run of bytes inside one record; it gives ids to the chunk
// of its first byte (it may run on into the next chunk).  piece_ids[c] lists, per chunk, the
// (record, count) of its pieces in byte order.
static void one_arena(int64_t n) {
    const int64_t N = n * LIST_CHUNK - (int64_t)below((uint32_t)LIST_CHUNK);  // a partial last chunk
    // record offsets: anywhere, with empty records and records of many chunks
    std::vector<uint64_t> off{0};
    while ((int64_t)off.back() < N) {
        const uint32_t kind = below(8);
        uint64_t len = kind == 0 ? 0 : kind == 1 ? 1 + below(40) : kind < 6 ? 1 + below(3000) : 1 + below(200000);
        if (off.back() + len > (uint64_t)N) len = (uint64_t)N - off.back();
        off.push_back(off.back() + len);
    }
    const int64_t R = (int64_t)off.size() - 1;
    // per byte: ids of the piece that starts there (0: none); long runs without ids; dense runs
    // of one id a byte (chunks of 1,024 ids)
    std::vector<uint8_t> ids_at((size_t)N, 0);
    for (int64_t p = 0; p < N;) {
        const uint32_t mode = below(6);
        const int64_t run = mode == 0 ? 1 + below(150000) : 1 + below(5000);
        for (int64_t q = p; q < p + run && q < N; ++q)
            ids_at[(size_t)q] = mode == 0 ? 0 : mode == 1 ? 1 : below(5) == 0 ? (uint8_t)(1 + below(3)) : 0;
        p += run;
    }
    // a chunk's list holds at most LIST_STRIDE ids
    std::vector<uint32_t> cnt((size_t)n, 0);
    for (int64_t p = 0; p < N; ++p) {
        uint32_t &c = cnt[(size_t)(p / LIST_CHUNK)];
        if (c + ids_at[(size_t)p] > (uint32_t)LIST_STRIDE) ids_at[(size_t)p] = 0;
        c += ids_at[(size_t)p];
    }
    std::vector<uint32_t> chunk_off((size_t)n + 1, 0);
    for (int64_t c = 0; c < n; ++c) chunk_off[(size_t)c + 1] = chunk_off[(size_t)c] + cnt[(size_t)c];
    // brute force: walk the bytes, id index t, the chunk and the position in its list
    uint32_t t = 0;
    int64_t r = 0;
    for (int64_t p = 0; p < N; ++p) {
        while (r < R && (int64_t)off[(size_t)r + 1] <= p) ++r;  // the record of byte p
        const int64_t c = p / LIST_CHUNK;
        for (int k = 0; k < ids_at[(size_t)p]; ++k, ++t) {
            const ListBracket br = list_bracket(off[(size_t)r], off[(size_t)r + 1], n);
            CHECK(br.lo <= c && c <= br.hi, "byte %lld record %lld bracket [%lld, %lld] chunk %lld", (long long)p,
                  (long long)r, (long long)br.lo, (long long)br.hi, (long long)c);
            const int64_t got = list_chunk_of(chunk_off.data(), br.lo, br.hi, t);
            CHECK(got == c, "id %u: chunk %lld, want %lld", t, (long long)got, (long long)c);
            // ... and from any chunk at or before it up to the arena's last (the rows' searches)
            const int64_t from = c - (int64_t)below((uint32_t)(c - br.lo) + 1);
            CHECK(list_chunk_of(chunk_off.data(), from, n - 1, t) == c, "id %u from chunk %lld", t, (long long)from);
            const int64_t slot = list_slot(chunk_off.data(), c, t);
            CHECK(slot >= c * LIST_STRIDE && slot < (c + 1) * LIST_STRIDE && slot - c * LIST_STRIDE == t - chunk_off[(size_t)c],
                  "id %u slot %lld", t, (long long)slot);
        }
    }
    CHECK(t == chunk_off[(size_t)n], "total %u", t);
    // brackets of records without bytes or ids stay inside the arena
    for (int64_t q = 0; q < R; ++q) {
        const ListBracket br = list_bracket(off[(size_t)q], off[(size_t)q + 1], n);
        CHECK(0 <= br.lo && br.lo <= br.hi && br.hi <= n - 1, "record %lld bracket [%lld, %lld]", (long long)q,
              (long long)br.lo, (long long)br.hi);
    }
}

int main() {
    const int64_t sizes[] = {1, 2, 3, 65, 200, 1000};
    for (int rep = 0; rep < 4; ++rep)
        for (int64_t n : sizes) one_arena(n);
    if (failures) {
        fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    printf("list_index ok\n");
    return 0;
}
