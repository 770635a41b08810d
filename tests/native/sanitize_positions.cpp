// Sanitizer driver for mmrag_lexicon_analyze_positions (tokenizer.cpp): built by tests/test_phrase_sanitizers.py with
// -fsanitize=address,undefined and with -fsanitize=thread and run on the CPU only.  The entry point splits a batch over
// its own worker threads; here several caller threads drive it at once, each on its own lexicon (a lexicon belongs to
// one caller at a time, as the Python wrapper holds it), through the capacity protocol's retry, and every result is
// checked against a plain restatement: the positions of a text's pairs rebuild its token sequence.
#include <ctype.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <random>
#include <string>
#include <thread>
#include <vector>

#include "../../include/mmrag.h"

// what common.hip provides inside the real library
namespace mmrag {
static thread_local char g_err[512];
void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
int num_cus() { return 256; }
}  // namespace mmrag

#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            exit(2);                                                    \
        }                                                               \
    } while (0)

static const char *WORDS[] = {"alpha", "beta", "gamma", "delta", "the", "of", "a", "x", "retrieval", "index"};
static const char *SEPS[] = {" ", "  ", ", ", ". ", "-", "\n", " ... "};

struct Batch {
    std::vector<uint32_t> cps;
    std::vector<int64_t> offsets;
    std::vector<std::vector<int>> words;   // per text: the word numbers in token order
};

static Batch make_batch(unsigned seed, int n_texts, int max_words) {
    std::mt19937 g(seed);
    Batch b;
    b.offsets.push_back(0);
    for (int i = 0; i < n_texts; ++i) {
        std::vector<int> seq;
        const int k = (int)(g() % (unsigned)(max_words + 1));
        for (int j = 0; j < k; ++j) {
            const int w = (int)(g() % 10u);
            seq.push_back(w);
            for (const char *p = WORDS[w]; *p; ++p) b.cps.push_back((uint32_t)(j % 3 == 0 ? toupper(*p) : *p));
            for (const char *p = SEPS[g() % 7u]; *p; ++p) b.cps.push_back((uint32_t)*p);
        }
        b.words.push_back(seq);
        b.offsets.push_back((int64_t)b.cps.size());
    }
    return b;
}

// one caller: its own lexicon, several batches, the retry from a capacity that is too small, n_threads workers inside
static void caller(unsigned seed, int n_threads) {
    void *lx = mmrag_lexicon_create();
    CHECK(lx);
    std::vector<int> word_of_id;   // term id -> word number, learnt from the first sighting
    for (int round = 0; round < 4; ++round) {
        const Batch b = make_batch(seed * 97u + (unsigned)round, 40 + 25 * round, 3000 / (1 + round));
        const int n = (int)b.words.size();
        std::vector<int64_t> out_off((size_t)n + 1);
        std::vector<int32_t> dl((size_t)n), ids(1), tfs(1), pos(1);
        int64_t needed = -1;
        // too small on purpose: the sizes come back, nothing is written past the capacities
        int st = mmrag_lexicon_analyze_positions(lx, b.cps.data(), b.offsets.data(), n, out_off.data(), ids.data(),
                                                 tfs.data(), dl.data(), 1, pos.data(), 1, &needed, n_threads);
        CHECK(st == MMRAG_EWORKSPACE || (st == MMRAG_OK && out_off[n] <= 1 && needed <= 1));
        int64_t total = 0;
        for (int i = 0; i < n; ++i) total += (int64_t)b.words[i].size();
        CHECK(needed == total);
        ids.assign((size_t)out_off[n] + 1, -1);
        tfs.assign((size_t)out_off[n] + 1, -1);
        pos.assign((size_t)needed + 1, -1);
        st = mmrag_lexicon_analyze_positions(lx, b.cps.data(), b.offsets.data(), n, out_off.data(), ids.data(),
                                             tfs.data(), dl.data(), out_off[n], pos.data(), needed, &needed, n_threads);
        CHECK(st == MMRAG_OK);
        CHECK(ids[(size_t)out_off[n]] == -1 && pos[(size_t)needed] == -1);   // the spare slots are untouched
        int64_t at = 0;
        for (int i = 0; i < n; ++i) {
            const std::vector<int> &want = b.words[i];
            CHECK(dl[i] == (int32_t)want.size());
            std::vector<int> got(want.size(), -1);
            int32_t prev_id = -1;
            for (int64_t j = out_off[i]; j < out_off[i + 1]; ++j) {
                CHECK(ids[j] > prev_id && tfs[j] >= 1);   // pairs sorted by id, distinct
                prev_id = ids[j];
                for (int32_t t = 0; t < tfs[j]; ++t, ++at) {
                    const int32_t p = pos[at];
                    CHECK(p >= 0 && p < (int32_t)want.size() && got[p] == -1);
                    CHECK(t == 0 || p > pos[at - 1]);     // ascending within a pair
                    if ((size_t)ids[j] >= word_of_id.size()) word_of_id.resize((size_t)ids[j] + 1, -1);
                    if (word_of_id[ids[j]] < 0) word_of_id[ids[j]] = want[p];
                    got[p] = word_of_id[ids[j]];
                }
            }
            CHECK(got == want);   // the positions rebuild the token sequence
        }
        CHECK(at == needed);
        CHECK(mmrag_lexicon_size(lx) <= 10);
    }
    mmrag_lexicon_destroy(lx);
}

int main() {
    std::vector<std::thread> th;
    for (unsigned t = 0; t < 6; ++t) th.emplace_back(caller, t + 1, 1 + (int)(t % 4) * 2);
    for (auto &t : th) t.join();
    // the null-pointer and empty cases
    void *lx = mmrag_lexicon_create();
    int64_t in_off = 0, out_off = -1, needed = -1;
    int32_t dl = -1;
    CHECK(mmrag_lexicon_analyze_positions(lx, nullptr, &in_off, 0, &out_off, nullptr, nullptr, &dl, 0, nullptr, 0,
                                          &needed, 4) == MMRAG_OK);
    CHECK(out_off == 0 && needed == 0);
    CHECK(mmrag_lexicon_analyze_positions(lx, nullptr, &in_off, 0, &out_off, nullptr, nullptr, &dl, 0, nullptr, 0,
                                          nullptr, 4) == MMRAG_EINVAL);
    mmrag_lexicon_destroy(lx);
    printf("sanitize_positions: ok\n");
    return 0;
}
