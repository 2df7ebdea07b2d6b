// Host check of csrc/wp_first.hpp: the first-piece table of the WordPiece chunk kernel's first
// probes, built with the header's own functions the way assets.cpp builds it (the same
// de-duplication: the last id of a duplicated piece wins), then looked up through them.  Every
// non-"##" piece of at most 14 bytes must be found with its id; no "##" payload, no longer piece
// cut to 14 bytes, no piece with one byte changed, added or dropped and no random lower-case
// string may be found unless it is itself such a piece.  The vocabulary is read from a file, one
// piece a line (the line number is the id); two synthetic vocabularies follow.
// Built and run by tests/test_wp_first.py.
#include "wp_first.hpp"

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <random>
#include <string>
#include <unordered_map>
#include <vector>

using namespace sdl;

static int fails = 0;
static long checked = 0;
static const char *what = "";
#define CHECK(c)                                                                             \
    do {                                                                                     \
        ++checked;                                                                           \
        if (!(c)) {                                                                          \
            if (fails++ < 20) printf("FAIL %s:%d %s  [%s]\n", __FILE__, __LINE__, #c, what); \
        }                                                                                    \
    } while (0)

struct Table {
    std::vector<WfSlot> slots;
    uint32_t mask = 0, seed = 0;
    int maxlen = 0;
    std::unordered_map<std::string, int> in;  // the pieces it holds -> id
    int lookup(const std::string &s) const {
        return wf_lookup(slots.data(), mask, seed, (const uint8_t *)s.data(), (int)s.size());
    }
};

static bool is_cont(const std::string &s) { return s.size() > 2 && s[0] == '#' && s[1] == '#'; }

static bool build(const std::vector<std::string> &pieces, Table &t) {
    std::unordered_map<std::string, int> last;
    for (size_t id = 0; id < pieces.size(); ++id) last[pieces[id]] = (int)id;
    std::vector<WfPiece> list;
    for (size_t id = 0; id < pieces.size(); ++id) {
        const std::string &s = pieces[id];
        if (s.empty() || last[s] != (int)id || is_cont(s)) continue;
        if (!wf_fits((const uint8_t *)s.data(), (int)s.size())) continue;
        list.push_back(WfPiece{(const uint8_t *)s.data(), (int)s.size(), (uint32_t)id});
        t.in[s] = (int)id;
        if ((int)s.size() > t.maxlen) t.maxlen = (int)s.size();
    }
    std::vector<std::vector<WfSlot>> tries;  // (every attempt's storage lives until the build returns)
    WfSlot *tab = nullptr;
    t.mask = wf_build(list.data(), (uint32_t)list.size(),
                      [&](uint32_t n) {
                          tries.emplace_back(n, WfSlot{{0, 0, 0, 0}});
                          return tries.back().data();
                      },
                      &t.seed, &tab);
    if (!t.mask) return false;
    t.slots.assign(tab, tab + t.mask + 1);
    return true;
}

// s must be found exactly when it is a piece of the table, and then with that piece's id
static void expect(const Table &t, const std::string &s) {
    const auto it = t.in.find(s);
    const int want = it == t.in.end() ? -1 : it->second;
    CHECK(t.lookup(s) == want);
}

static void check_vocab(const std::vector<std::string> &pieces, const char *name, size_t min_in) {
    what = name;
    Table t;
    const bool built = build(pieces, t);
    CHECK(built);
    if (!built) return;
    const size_t slots = (size_t)t.mask + 1;
    printf("%s: %zu pieces, %zu in the table, %zu slots (%zu KiB), load %.3f, seed %u, longest %d\n", name,
           pieces.size(), t.in.size(), slots, slots * sizeof(WfSlot) >> 10, (double)t.in.size() / slots, t.seed,
           t.maxlen);
    CHECK(t.in.size() >= min_in);
    CHECK((slots & t.mask) == 0 && slots <= WF_MAX_SLOTS);
    CHECK(t.in.size() * 100 <= slots * 45);
    CHECK(t.maxlen <= WF_MAXLEN);
    // the table holds these pieces and nothing else
    size_t used = 0;
    for (const WfSlot &s : t.slots) used += !wf_empty(s);
    CHECK(used == t.in.size());
    for (const auto &kv : t.in) CHECK(t.lookup(kv.first) == kv.second);
    // (the last id of a duplicated piece)
    for (size_t id = 0; id < pieces.size(); ++id) {
        const auto it = t.in.find(pieces[id]);
        if (it != t.in.end()) CHECK(it->second >= (int)id);
    }
    for (const std::string &s : pieces) {
        if (s.empty()) continue;
        const bool cont = is_cont(s);
        const std::string pay = cont ? s.substr(2) : s;
        if (cont) expect(t, pay);                                       // a "##" payload
        if (!cont && s.size() > (size_t)WF_MAXLEN) expect(t, s.substr(0, WF_MAXLEN));  // a longer piece, cut
        if (!cont) expect(t, s);
        for (size_t i = 0; i <= pay.size(); ++i) {
            for (char c : {'a', 'e', 's', '1', '#'}) {  // one byte added
                std::string x = pay;
                x.insert(i, 1, c);
                expect(t, x);
            }
            if (i == pay.size()) break;
            std::string d = pay;  // one byte dropped
            d.erase(i, 1);
            if (!d.empty()) expect(t, d);
            for (int delta : {1, 32, -1}) {  // one byte changed
                std::string x = pay;
                x[i] = (char)(x[i] + delta);
                if (x[i] != 0) expect(t, x);
            }
        }
    }
    std::mt19937 rng(12345);
    for (int k = 0; k < 100000; ++k) {
        std::string x(1 + rng() % WF_MAXLEN, 'a');
        for (char &c : x) c = (char)('a' + rng() % 26);
        expect(t, x);
    }
    // what never stands in a slot is never found
    CHECK(t.lookup("") == -1);
    CHECK(t.lookup(std::string("a\0b", 3)) == -1);
    CHECK(t.lookup(std::string(15, 'a')) == -1);
}

int main(int argc, char **argv) {
    if (argc != 2) {
        printf("usage: wp_first_check <pieces file>\n");
        return 2;
    }
    std::vector<std::string> pieces;
    {
        std::ifstream f(argv[1], std::ios::binary);
        std::string line;
        while (std::getline(f, line)) pieces.push_back(line);
    }
    if (pieces.size() < 1000) {
        printf("FAIL: %zu pieces read from %s\n", pieces.size(), argv[1]);
        return 2;
    }
    check_vocab(pieces, "proxy vocabulary", 20000);

    // duplicates (the last id wins, also across a "##" piece in between), a 14-byte piece that
    // is the prefix of a 15-byte one, a piece with a zero byte, empty pieces
    const std::string p14 = "abcdefghijklmn";
    std::vector<std::string> syn = {"[PAD]", "[UNK]", "the", "##the", "the", "of", p14, p14 + "o", "##" + p14, "of",
                                    "", "the", std::string("a\0b", 3), "a", "b", "##a", p14 + "op", "#", "##", "###"};
    for (int k = 0; k < 300; ++k) syn.push_back("w" + std::to_string(k * 7919 % 1000));  // (with duplicates)
    check_vocab(syn, "synthetic: duplicates and prefixes", 100);
    // only [UNK] is short enough for the table
    std::vector<std::string> lone = {"[PAD]andsomethingelse", "[UNK]", "##s", "##ing", "internationalization",
                                     "##abcdefghijklmn", "characteristically"};
    check_vocab(lone, "synthetic: only [UNK]", 1);

    if (fails) {
        printf("wp_first FAILED: %d of %ld checks\n", fails, checked);
        return 1;
    }
    printf("wp_first ok: %ld checks\n", checked);
    return 0;
}
