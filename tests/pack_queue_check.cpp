// Host check of csrc/pack_queue.hpp (built and run by tests/test_pack_model.py with the host
// compiler's address and undefined-behaviour sanitizers): a queue of batches of B rows is played
// over random sequences of calls that emit G rows each -- G = 0, G below, at and far above B --
// copying the rows where the plan says, as the library copies them from the device planes.  The
// batches handed out, read in order, must hold every row once, in order, and every copy must stay
// inside its source and its batch (the sanitizers watch the buffers).
#include "pack_queue.hpp"

#include <cstdio>
#include <deque>
#include <memory>
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

struct Batch {
    std::vector<uint64_t> row;  // exactly B slots: a write past them is the sanitizer's to find
    uint32_t rows = 0;
    explicit Batch(uint32_t B) : row(B, ~0ull) {}
};

static void one_stream(uint32_t B, int calls) {
    std::deque<std::unique_ptr<Batch>> out;  // full batches, in order
    std::unique_ptr<Batch> work(new Batch(B));
    uint64_t next_row = 0, popped = 0;
    for (int c = 0; c < calls; ++c) {
        const uint32_t kind = below(6);
        const uint64_t G = kind == 0 ? 0 : kind == 1 ? 1 : kind == 2 ? B - work->rows : kind == 3 ? B : kind == 4
                           ? below(3 * B + 1) : (uint64_t)B * (1 + below(40)) + below(B);
        std::vector<uint64_t> dev((size_t)G);  // the call's rows, as the device planes hold them
        for (uint64_t g = 0; g < G; ++g) dev[(size_t)g] = next_row + g;
        const PackPlan plan = pack_queue_plan(work->rows, B, G);
        std::vector<std::unique_ptr<Batch>> bs;
        bs.push_back(std::move(work));
        while (bs.size() < (size_t)plan.completed + 1) bs.emplace_back(new Batch(B));
        uint64_t covered = 0;
        for (const PackSeg &s : plan.segs) {
            CHECK(s.batch < bs.size(), "segment for batch %u of %zu", s.batch, bs.size());
            CHECK(s.n > 0 && (uint64_t)s.dst + s.n <= B, "segment rows [%u, +%u) of a batch of %u", s.dst, s.n, B);
            CHECK(s.g0 == covered && (uint64_t)s.g0 + s.n <= G, "segment source [%u, +%u) of %llu", s.g0, s.n,
                  (unsigned long long)G);
            if (failures) return;
            Batch &b = *bs[s.batch];
            CHECK(b.rows == s.dst, "batch %u holds %u rows, segment starts at %u", s.batch, b.rows, s.dst);
            for (uint32_t i = 0; i < s.n; ++i) b.row[s.dst + i] = dev[(size_t)s.g0 + i];
            b.rows += s.n;
            covered += s.n;
        }
        CHECK(covered == G, "%llu of %llu rows placed", (unsigned long long)covered, (unsigned long long)G);
        for (uint32_t k = 0; k < plan.completed; ++k) {
            CHECK(bs[k]->rows == B, "batch %u queued with %u rows", k, bs[k]->rows);
            out.push_back(std::move(bs[k]));
        }
        CHECK(bs.back()->rows == plan.fill && plan.fill < B, "working batch %u rows, plan %u", bs.back()->rows, plan.fill);
        work = std::move(bs.back());
        next_row += G;
        // the consumer pops some of the queue between calls
        for (uint32_t n = below(4); n > 0 && !out.empty(); --n) {
            for (uint32_t i = 0; i < B; ++i, ++popped)
                CHECK(out.front()->row[i] == popped, "row %llu came out as %llu", (unsigned long long)popped,
                      (unsigned long long)out.front()->row[i]);
            out.pop_front();
        }
    }
    for (; !out.empty(); out.pop_front())
        for (uint32_t i = 0; i < B; ++i, ++popped)
            CHECK(out.front()->row[i] == popped, "row %llu came out as %llu", (unsigned long long)popped,
                  (unsigned long long)out.front()->row[i]);
    for (uint32_t i = 0; i < work->rows; ++i, ++popped)
        CHECK(work->row[i] == popped, "working row %llu is %llu", (unsigned long long)popped,
              (unsigned long long)work->row[i]);
    CHECK(popped == next_row, "%llu rows out for %llu in", (unsigned long long)popped, (unsigned long long)next_row);
}

int main() {
    const uint32_t sizes[] = {1, 2, 3, 4, 7, 128, 4096};
    for (int rep = 0; rep < 8; ++rep)
        for (uint32_t B : sizes) one_stream(B, B > 1000 ? 12 : 200);
    // states the queue is never in plan nothing
    CHECK(pack_queue_plan(4, 4, 10).segs.empty() && pack_queue_plan(0, 0, 10).segs.empty(), "bad state planned rows");
    if (failures) {
        fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    printf("pack_queue ok\n");
    return 0;
}
