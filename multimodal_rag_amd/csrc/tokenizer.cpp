// Native WordPiece tokenizer (host, multi-threaded): the step in front of mmrag_encoder_forward.
//
// The reference tokenises inside SentenceTransformer.encode (app/utils/embedder.py:397-403), i.e. with
// Hugging Face `tokenizers` (native code).  The Python restatement in multimodal_rag_amd/tokenizer.py
// (pinned against transformers.BertTokenizer) does ~500 chunks/s per core, 30x below what one MI355X
// embeds, so ingest needs this: BERT BasicTokenizer (clean, CJK spacing, whitespace split, lower-case,
// NFD + strip Mn, punctuation split) + greedy longest-match WordPiece, on UTF-32 input, with a thread
// per slice of the batch.  Unicode data comes from unicode_tables.inc, generated from the same
// interpreter's unicodedata that tokenizer.py uses; tests/test_tokenizer.py fuzzes the two against
// each other.
#include <limits.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <thread>
#include <vector>

#include "mmrag_internal.h"

namespace {

#include "unicode_tables.inc"

template <size_t N>
inline bool in_ranges(const uint32_t (&r)[N][2], uint32_t cp) {
    size_t lo = 0, hi = N;
    while (lo < hi) {
        const size_t mid = (lo + hi) / 2;
        if (cp > r[mid][1])
            lo = mid + 1;
        else if (cp < r[mid][0])
            hi = mid;
        else
            return true;
    }
    return false;
}

template <size_t N, size_t W>
inline const uint32_t *find_map(const uint32_t (&m)[N][W], uint32_t cp) {
    size_t lo = 0, hi = N;
    while (lo < hi) {
        const size_t mid = (lo + hi) / 2;
        if (m[mid][0] < cp)
            lo = mid + 1;
        else
            hi = mid;
    }
    return (lo < N && m[lo][0] == cp) ? m[lo] : nullptr;
}

inline bool is_cjk(uint32_t cp) {
    return (cp >= 0x4E00 && cp <= 0x9FFF) || (cp >= 0x3400 && cp <= 0x4DBF) || (cp >= 0x20000 && cp <= 0x2A6DF) ||
           (cp >= 0x2A700 && cp <= 0x2B73F) || (cp >= 0x2B740 && cp <= 0x2B81F) || (cp >= 0x2B820 && cp <= 0x2CEAF) ||
           (cp >= 0xF900 && cp <= 0xFAFF) || (cp >= 0x2F800 && cp <= 0x2FA1F);
}

inline bool is_punct(uint32_t cp) {
    if ((cp >= 33 && cp <= 47) || (cp >= 58 && cp <= 64) || (cp >= 91 && cp <= 96) || (cp >= 123 && cp <= 126)) return true;
    return cp >= 128 && in_ranges(RANGES_PUNCT, cp);
}

typedef std::vector<uint32_t> u32s;

// str.lower() of one word (context-free table + CPython's final-sigma rule)
void lower_word(const u32s &w, u32s &out) {
    out.clear();
    const size_t n = w.size();
    for (size_t i = 0; i < n; ++i) {
        const uint32_t c = w[i];
        if (c < 128) {
            out.push_back((c >= 'A' && c <= 'Z') ? c + 32 : c);
            continue;
        }
        if (c == 0x3A3) {
            long j = (long)i - 1;
            while (j >= 0 && in_ranges(RANGES_CASE_IGN, w[j])) --j;
            bool fin = j >= 0 && in_ranges(RANGES_CASED, w[j]);
            if (fin) {
                size_t k = i + 1;
                while (k < n && in_ranges(RANGES_CASE_IGN, w[k])) ++k;
                fin = k == n || !in_ranges(RANGES_CASED, w[k]);
            }
            out.push_back(fin ? 0x3C2 : 0x3C3);
            continue;
        }
        if (const uint32_t *m = find_map(MAP_LOWER, c)) {
            for (uint32_t t = 0; t < m[1]; ++t) out.push_back(m[2 + t]);
        } else if (const uint32_t *m4 = find_map(MAP_LOWER4, c)) {
            for (uint32_t t = 0; t < 4; ++t) out.push_back(m4[2 + t]);
        } else {
            out.push_back(c);
        }
    }
}

inline uint32_t ccc_of(uint32_t cp) {
    if (cp < 0x300) return 0;
    const uint32_t *m = find_map(MAP_CCC, cp);
    return m ? m[1] : 0;
}

// unicodedata.normalize("NFD", w), with the Mn characters dropped afterwards when strip_mn is set
void nfd(const u32s &w, u32s &out, u32s &tmp, bool strip_mn) {
    tmp.clear();
    for (uint32_t c : w) {
        if (c < 0xC0) {
            tmp.push_back(c);
        } else if (c >= 0xAC00 && c <= 0xD7A3) {  // Hangul syllable: algorithmic decomposition
            const uint32_t s = c - 0xAC00;
            tmp.push_back(0x1100 + s / 588);
            tmp.push_back(0x1161 + (s % 588) / 28);
            if (s % 28) tmp.push_back(0x11A7 + s % 28);
        } else if (const uint32_t *m = find_map(MAP_NFD, c)) {
            for (uint32_t t = 0; t < m[1]; ++t) tmp.push_back(m[2 + t]);
        } else if (const uint32_t *m4 = find_map(MAP_NFD4, c)) {
            for (uint32_t t = 0; t < 4; ++t) tmp.push_back(m4[2 + t]);
        } else {
            tmp.push_back(c);
        }
    }
    // canonical ordering: stable sort of every run of combining marks by combining class
    for (size_t i = 0; i < tmp.size();) {
        if (ccc_of(tmp[i]) == 0) {
            ++i;
            continue;
        }
        size_t j = i;
        while (j < tmp.size() && ccc_of(tmp[j]) != 0) ++j;
        if (j - i > 1)
            std::stable_sort(tmp.begin() + i, tmp.begin() + j, [](uint32_t a, uint32_t b) { return ccc_of(a) < ccc_of(b); });
        i = j;
    }
    out.clear();
    for (uint32_t c : tmp)
        if (!strip_mn || !(c >= 0x300 && in_ranges(RANGES_MN, c))) out.push_back(c);
}

void nfd_strip_mn(const u32s &w, u32s &out, u32s &tmp) { nfd(w, out, tmp, true); }

struct Vocab {
    // open-addressing table over (codepoint string -> id); `first` = whole entries, `cont` = entries that
    // start with "##", keyed by what follows the prefix
    struct Table {
        std::vector<uint32_t> pool;
        struct Slot {
            uint64_t hash;
            uint32_t off, len;
            int32_t id;
        };
        std::vector<Slot> slots;
        size_t mask = 0;
        static uint64_t hash_of(const uint32_t *p, size_t n) {
            uint64_t h = 1469598103934665603ull;
            for (size_t i = 0; i < n; ++i) {
                h ^= p[i];
                h *= 1099511628211ull;
            }
            return h | 1;  // 0 marks an empty slot
        }
        void build(const std::vector<std::pair<u32s, int32_t>> &items) {
            size_t cap = 16;
            while (cap < items.size() * 2 + 2) cap <<= 1;
            slots.assign(cap, Slot{0, 0, 0, -1});
            mask = cap - 1;
            for (const auto &it : items) {
                const uint64_t h = hash_of(it.first.data(), it.first.size());
                size_t i = h & mask;
                bool dup = false;
                while (slots[i].hash) {
                    if (slots[i].hash == h && slots[i].len == it.first.size() &&
                        !memcmp(&pool[slots[i].off], it.first.data(), it.first.size() * 4)) {
                        slots[i].id = it.second;  // a later duplicate line wins, as a Python dict would
                        dup = true;
                        break;
                    }
                    i = (i + 1) & mask;
                }
                if (dup) continue;
                slots[i] = Slot{h, (uint32_t)pool.size(), (uint32_t)it.first.size(), it.second};
                pool.insert(pool.end(), it.first.begin(), it.first.end());
            }
        }
        int32_t find(const uint32_t *p, size_t n) const {
            if (slots.empty()) return -1;
            const uint64_t h = hash_of(p, n);
            size_t i = h & mask;
            while (slots[i].hash) {
                if (slots[i].hash == h && slots[i].len == n && !memcmp(&pool[slots[i].off], p, n * 4)) return slots[i].id;
                i = (i + 1) & mask;
            }
            return -1;
        }
    };
    Table first, cont;
    int32_t cls = 101, sep = 102, unk = 100;
    int lower = 1;
    int max_chars = 100;
};

void wordpiece(const Vocab &v, const u32s &word, std::vector<int32_t> &ids) {
    const size_t n = word.size();
    if ((int)n > v.max_chars) {
        ids.push_back(v.unk);
        return;
    }
    const size_t mark = ids.size();
    size_t start = 0;
    while (start < n) {
        size_t end = n;
        int32_t cur = -1;
        while (start < end) {
            cur = (start == 0 ? v.first : v.cont).find(&word[start], end - start);
            if (cur >= 0) break;
            --end;
        }
        if (cur < 0) {
            ids.resize(mark);
            ids.push_back(v.unk);
            return;
        }
        ids.push_back(cur);
        start = end;
    }
}

// the WordPiece ids of `text` appended to `ids`, stopping once ids holds `stop` entries (it may hold a few more)
void pieces(const Vocab &v, const uint32_t *text, size_t n, int stop, std::vector<int32_t> &ids) {
    u32s word, low, norm, tmp, piece;
    auto flush_piece = [&]() {
        if (!piece.empty()) {
            wordpiece(v, piece, ids);
            piece.clear();
        }
    };
    auto flush_word = [&]() -> bool {  // false: enough ids
        if (word.empty()) return true;
        const u32s *w = &word;
        if (v.lower) {
            lower_word(word, low);
            nfd_strip_mn(low, norm, tmp);
            w = &norm;
        }
        // punctuation split.  tokenizer.py checks the id budget once per basic token.
        for (uint32_t c : *w) {
            if (is_punct(c)) {
                flush_piece();
                if ((int)ids.size() >= stop) break;
                piece.push_back(c);
                flush_piece();
                if ((int)ids.size() >= stop) break;
            } else {
                piece.push_back(c);
            }
        }
        if ((int)ids.size() < stop) flush_piece();
        piece.clear();
        word.clear();
        return (int)ids.size() < stop;
    };
    bool more = true;
    for (size_t i = 0; i < n && more; ++i) {
        const uint32_t c = text[i];
        if (c == 0 || c == 0xFFFD) continue;
        const bool ws = c == ' ' || c == '\t' || c == '\n' || c == '\r';
        if (!ws && (c < 0x20 || (c >= 0x7F && in_ranges(RANGES_CTRL, c)))) continue;  // Cc / Cf
        if (ws || (c >= 0xA0 && in_ranges(RANGES_ZS, c)) || c == 0x2028 || c == 0x2029 || c == 0x1C || c == 0x1D ||
            c == 0x1E || c == 0x1F || c == 0x85) {
            more = flush_word();
        } else if (is_cjk(c)) {
            more = flush_word();
            if (more) {
                word.push_back(c);
                more = flush_word();
            }
        } else {
            word.push_back(c);
        }
    }
    if (more) flush_word();
}

void encode_one(const Vocab &v, const uint32_t *text, size_t n, int max_length, int32_t *out, int32_t *out_len) {
    std::vector<int32_t> ids;
    ids.reserve((size_t)max_length + 8);
    ids.push_back(v.cls);
    const int stop = max_length - 1;
    pieces(v, text, n, stop, ids);
    int len = (int)ids.size();
    if (len > stop) len = stop;
    for (int i = 0; i < len; ++i) out[i] = ids[i];
    out[len] = v.sep;
    *out_len = len + 1;
}

// lengths kept of a pair of piece lists under `budget` tokens: the fast tokenizer's TruncationStrategy::LongestFirst
void longest_first(int la, int lb, int budget, int *ka, int *kb) {
    if (la + lb <= budget) {
        *ka = la, *kb = lb;
    } else if (la <= lb && la <= budget / 2) {
        *ka = la, *kb = budget - la;
    } else if (lb < la && lb <= budget / 2) {
        *ka = budget - lb, *kb = lb;
    } else {
        const int h = budget / 2;
        *ka = la > lb ? budget - h : h;
        *kb = budget - *ka;
    }
}

// fn(lo, hi) over [0, n) on up to n_threads threads, one contiguous slice each
template <class F>
void parallel_slices(int n, int n_threads, F fn) {
    if (n_threads > n) n_threads = n > 0 ? n : 1;
    if (n_threads <= 1) {
        fn(0, n);
        return;
    }
    std::vector<std::thread> th;
    const int per = (n + n_threads - 1) / n_threads;
    for (int t = 0; t < n_threads; ++t) {
        const int lo = t * per, hi = std::min(n, lo + per);
        if (lo < hi) th.emplace_back(fn, lo, hi);
    }
    for (auto &t : th) t.join();
}

// ---- BM25 word analyzer and lexicon ------------------------------------------------------------------------------
// The terms of one text: BERT's cleaning, whitespace split and CJK spacing (as `pieces`), then per word str.lower()
// and the canonical decomposition WITH its combining marks ("học" != "hoc"), split at punctuation, which is dropped.
// Term i of the text is pool[ends[i-1] .. ends[i]) (ends[-1] = 0).
struct Analyzed {
    u32s pool;
    std::vector<uint32_t> ends;
    std::vector<int32_t> ids;   // term ids in token order (-1: not in the lexicon)
};

void analyze_text(const uint32_t *text, size_t n, Analyzed &a) {
    a.pool.clear();
    a.ends.clear();
    u32s word, low, norm, tmp;
    auto flush_word = [&]() {
        if (word.empty()) return;
        lower_word(word, low);
        nfd(low, norm, tmp, false);
        size_t start = a.pool.size();
        for (uint32_t c : norm) {
            if (is_punct(c)) {
                if (a.pool.size() > start) a.ends.push_back((uint32_t)a.pool.size());
                start = a.pool.size();
            } else {
                a.pool.push_back(c);
            }
        }
        if (a.pool.size() > start) a.ends.push_back((uint32_t)a.pool.size());
        word.clear();
    };
    for (size_t i = 0; i < n; ++i) {
        const uint32_t c = text[i];
        if (c == 0 || c == 0xFFFD) continue;
        const bool ws = c == ' ' || c == '\t' || c == '\n' || c == '\r';
        if (!ws && (c < 0x20 || (c >= 0x7F && in_ranges(RANGES_CTRL, c)))) continue;  // Cc / Cf
        if (ws || (c >= 0xA0 && in_ranges(RANGES_ZS, c)) || c == 0x2028 || c == 0x2029 || c == 0x1C || c == 0x1D ||
            c == 0x1E || c == 0x1F || c == 0x85) {
            flush_word();
        } else if (is_cjk(c)) {
            flush_word();
            word.push_back(c);
            flush_word();
        } else {
            word.push_back(c);
        }
    }
    flush_word();
}

// term string -> int32 id in first-seen order: a growable open-addressing table over one code-point pool
struct Lexicon {
    struct Slot {
        uint64_t hash;
        uint64_t off;
        uint32_t len;
        int32_t id;
    };
    u32s pool;
    std::vector<uint64_t> starts;   // term id's code points are pool[starts[id] .. starts[id + 1]) (the pool's end for the last)
    std::vector<Slot> slots;
    size_t mask;
    int32_t n = 0;
    Lexicon() : slots(1024, Slot{0, 0, 0, -1}), mask(1023) {}

    int32_t find(const uint32_t *p, size_t len) const {
        const uint64_t h = Vocab::Table::hash_of(p, len);
        for (size_t i = h & mask; slots[i].hash; i = (i + 1) & mask)
            if (slots[i].hash == h && slots[i].len == len && !memcmp(&pool[slots[i].off], p, len * 4)) return slots[i].id;
        return -1;
    }
    int32_t insert(const uint32_t *p, size_t len) {
        const int32_t got = find(p, len);
        if (got >= 0) return got;
        if ((size_t)(n + 1) * 2 > slots.size()) {
            std::vector<Slot> old;
            old.swap(slots);
            slots.assign(old.size() * 2, Slot{0, 0, 0, -1});
            mask = slots.size() - 1;
            for (const Slot &s : old) {
                if (!s.hash) continue;
                size_t i = s.hash & mask;
                while (slots[i].hash) i = (i + 1) & mask;
                slots[i] = s;
            }
        }
        const uint64_t h = Vocab::Table::hash_of(p, len);
        size_t i = h & mask;
        while (slots[i].hash) i = (i + 1) & mask;
        slots[i] = Slot{h, (uint64_t)pool.size(), (uint32_t)len, n};
        starts.push_back((uint64_t)pool.size());
        pool.insert(pool.end(), p, p + len);
        return n++;
    }
};

}  // namespace

using namespace mmrag;

extern "C" {

// vocab: `n_tokens` UTF-32 strings concatenated in `cps`, token i = cps[offsets[i] .. offsets[i+1]); id = i.
void *mmrag_wordpiece_create(const uint32_t *cps, const int64_t *offsets, int n_tokens, int lower) {
    if (!cps || !offsets || n_tokens <= 0) {
        set_error("wordpiece_create: empty vocabulary");
        return nullptr;
    }
    Vocab *v = new Vocab();
    v->lower = lower;
    std::vector<std::pair<u32s, int32_t>> first, cont;
    first.reserve(n_tokens);
    for (int i = 0; i < n_tokens; ++i) {
        u32s t(cps + offsets[i], cps + offsets[i + 1]);
        if (t.size() > 2 && t[0] == '#' && t[1] == '#') cont.emplace_back(u32s(t.begin() + 2, t.end()), i);
        first.emplace_back(std::move(t), i);
    }
    v->first.build(first);
    v->cont.build(cont);
    auto special = [&](const char *s, int32_t dflt) {
        u32s k;
        for (const char *p = s; *p; ++p) k.push_back((uint32_t)*p);
        const int32_t id = v->first.find(k.data(), k.size());
        return id >= 0 ? id : dflt;
    };
    v->cls = special("[CLS]", 101);
    v->sep = special("[SEP]", 102);
    v->unk = special("[UNK]", 100);
    return v;
}

void mmrag_wordpiece_destroy(void *tk) { delete (Vocab *)tk; }

// texts: n UTF-32 strings concatenated (text i = cps[offsets[i] .. offsets[i+1])).
// ids [n, max_length] int32 (rows are [CLS] ... [SEP], the rest untouched), lens [n].
int mmrag_wordpiece_encode_batch(const void *tk, const uint32_t *cps, const int64_t *offsets, int n, int max_length,
                                 int32_t *ids, int32_t *lens, int n_threads) {
    MMRAG_CHECK_ARG(tk && offsets && ids && lens, "wordpiece_encode_batch: null pointer");
    MMRAG_CHECK_ARG(n >= 0 && max_length >= 2, "wordpiece_encode_batch: bad shape n=%d max_length=%d", n, max_length);
    const Vocab &v = *(const Vocab *)tk;
    if (n_threads < 1) n_threads = 1;
    if (n_threads > n) n_threads = n > 0 ? n : 1;
    // a thread is worth starting for ~16 k code points (a 256-query batch of one-line queries is faster on ONE thread:
    // 0.28 ms against 0.53 ms on eight, all of the difference thread start-up)
    if (n > 0) {
        const int64_t by_work = 1 + (offsets[n] - offsets[0]) / 16384;
        if (n_threads > by_work) n_threads = (int)by_work;
    }
    auto work = [&](int lo, int hi) {
        for (int i = lo; i < hi; ++i)
            encode_one(v, cps + offsets[i], (size_t)(offsets[i + 1] - offsets[i]), max_length,
                       ids + (size_t)i * max_length, lens + i);
    };
    if (n_threads == 1) {
        work(0, n);
        return MMRAG_OK;
    }
    std::vector<std::thread> th;
    const int per = (n + n_threads - 1) / n_threads;
    for (int t = 0; t < n_threads; ++t) {
        const int lo = t * per, hi = std::min(n, lo + per);
        if (lo < hi) th.emplace_back(work, lo, hi);
    }
    for (auto &t : th) t.join();
    return MMRAG_OK;
}

// pairs i = (a_i, b_i): [CLS] a [SEP] b [SEP], type ids 0 through the first [SEP], 1 after it; LongestFirst truncation
// of the pieces to max_length - 3.  Each side is tokenised in full (the rule compares the untruncated lengths); a text
// equal to the previous pair's text on the same side is not tokenised again (the query of a rerank batch).
int mmrag_wordpiece_encode_pairs(const void *tk, const uint32_t *cps_a, const int64_t *offsets_a, const uint32_t *cps_b,
                                 const int64_t *offsets_b, int n, int max_length, int32_t *ids, int32_t *type_ids,
                                 int32_t *lens, int n_threads) {
    MMRAG_CHECK_ARG(tk && offsets_a && offsets_b && ids && type_ids && lens, "wordpiece_encode_pairs: null pointer");
    MMRAG_CHECK_ARG(n >= 0 && max_length >= 3, "wordpiece_encode_pairs: bad shape n=%d max_length=%d", n, max_length);
    MMRAG_CHECK_ARG(n == 0 || ((cps_a || offsets_a[n] == offsets_a[0]) && (cps_b || offsets_b[n] == offsets_b[0])),
                    "wordpiece_encode_pairs: null text");
    const Vocab &v = *(const Vocab *)tk;
    if (n_threads < 1) n_threads = 1;
    if (n_threads > n) n_threads = n > 0 ? n : 1;
    if (n > 0) {   // as mmrag_wordpiece_encode_batch: a thread per ~16 k code points
        const int64_t by_work = 1 + (offsets_a[n] - offsets_a[0] + offsets_b[n] - offsets_b[0]) / 16384;
        if (n_threads > by_work) n_threads = (int)by_work;
    }
    const int budget = max_length - 3;
    auto same_as_prev = [](const uint32_t *cps, const int64_t *off, int i) {
        const int64_t n0 = off[i] - off[i - 1], n1 = off[i + 1] - off[i];
        return n0 == n1 && std::equal(cps + off[i - 1], cps + off[i], cps + off[i]);
    };
    auto work = [&](int lo, int hi) {
        std::vector<int32_t> pa, pb;
        for (int i = lo; i < hi; ++i) {
            if (i == lo || !same_as_prev(cps_a, offsets_a, i)) {
                pa.clear();
                pieces(v, cps_a + offsets_a[i], (size_t)(offsets_a[i + 1] - offsets_a[i]), INT_MAX, pa);
            }
            if (i == lo || !same_as_prev(cps_b, offsets_b, i)) {
                pb.clear();
                pieces(v, cps_b + offsets_b[i], (size_t)(offsets_b[i + 1] - offsets_b[i]), INT_MAX, pb);
            }
            int ka, kb;
            longest_first((int)pa.size(), (int)pb.size(), budget, &ka, &kb);
            int32_t *o = ids + (size_t)i * max_length, *ty = type_ids + (size_t)i * max_length;
            int at = 0;
            o[at] = v.cls, ty[at++] = 0;
            for (int j = 0; j < ka; ++j) o[at] = pa[j], ty[at++] = 0;
            o[at] = v.sep, ty[at++] = 0;
            for (int j = 0; j < kb; ++j) o[at] = pb[j], ty[at++] = 1;
            o[at] = v.sep, ty[at++] = 1;
            lens[i] = at;
        }
    };
    if (n_threads == 1) {
        work(0, n);
        return MMRAG_OK;
    }
    std::vector<std::thread> th;
    const int per = (n + n_threads - 1) / n_threads;
    for (int t = 0; t < n_threads; ++t) {
        const int lo = t * per, hi = std::min(n, lo + per);
        if (lo < hi) th.emplace_back(work, lo, hi);
    }
    for (auto &t : th) t.join();
    return MMRAG_OK;
}

void *mmrag_lexicon_create(void) { return new Lexicon(); }

void mmrag_lexicon_destroy(void *lexicon) { delete (Lexicon *)lexicon; }

int64_t mmrag_lexicon_size(const void *lexicon) { return lexicon ? ((const Lexicon *)lexicon)->n : -1; }

// Analysis on n_threads threads (a thread per ~16 k code points, as mmrag_wordpiece_encode_batch); only the insertion
// of unseen terms runs on one thread, in text order, so ids are first-seen whatever the thread count.
// The body of mmrag_lexicon_analyze_batch and mmrag_lexicon_analyze_positions (`name`, for error texts).  With
// want_positions every pair's token positions are written too: ascending, concatenated in pair order, sum(dl) ints.
static int analyze_batch_impl(const char *name, void *lexicon, const uint32_t *cps, const int64_t *offsets, int n,
                              int mode, int64_t *out_offsets, int32_t *term_ids, int32_t *tfs, int32_t *dl,
                              int64_t capacity, bool want_positions, int32_t *positions, int64_t pos_capacity,
                              int64_t *pos_needed, int n_threads) {
    MMRAG_CHECK_ARG(lexicon && offsets && out_offsets && dl, "%s: null pointer", name);
    MMRAG_CHECK_ARG(n >= 0, "%s: n=%d", name, n);
    MMRAG_CHECK_ARG(mode == MMRAG_LEX_DOCUMENTS || mode == MMRAG_LEX_QUERIES, "%s: bad mode %d", name, mode);
    MMRAG_CHECK_ARG(n == 0 || cps || offsets[n] == offsets[0], "%s: null text", name);
    MMRAG_CHECK_ARG(capacity >= 0 && (capacity == 0 || (term_ids && tfs)), "%s: null output", name);
    MMRAG_CHECK_ARG(!want_positions || (pos_needed && pos_capacity >= 0 && (pos_capacity == 0 || positions)),
                    "%s: null positions", name);
    Lexicon &lx = *(Lexicon *)lexicon;
    if (n_threads < 1) n_threads = 1;
    if (n > 0) {
        const int64_t by_work = 1 + (offsets[n] - offsets[0]) / 16384;
        if (n_threads > by_work) n_threads = (int)by_work;
    }
    std::vector<Analyzed> docs((size_t)n);
    // 1. split and normalise; look every term up (read-only: no insertion runs meanwhile)
    parallel_slices(n, n_threads, [&](int lo, int hi) {
        for (int i = lo; i < hi; ++i) {
            Analyzed &a = docs[i];
            analyze_text(cps + offsets[i], (size_t)(offsets[i + 1] - offsets[i]), a);
            a.ids.resize(a.ends.size());
            for (size_t t = 0, b = 0; t < a.ends.size(); b = a.ends[t++]) a.ids[t] = lx.find(&a.pool[b], a.ends[t] - b);
        }
    });
    // 2. documents: unseen terms get ids in text order
    if (mode == MMRAG_LEX_DOCUMENTS) {
        for (Analyzed &a : docs)
            for (size_t t = 0, b = 0; t < a.ends.size(); b = a.ends[t++])
                if (a.ids[t] < 0) a.ids[t] = lx.insert(&a.pool[b], a.ends[t] - b);
    }
    // 3. (term id, tf) pairs: documents sorted by id, queries in order of first occurrence; unknown terms dropped
    std::vector<std::vector<std::pair<int32_t, int32_t>>> pairs((size_t)n);
    std::vector<std::vector<int32_t>> where((size_t)(want_positions ? n : 0));   // positions, in pair order
    parallel_slices(n, n_threads, [&](int lo, int hi) {
        std::vector<int32_t> sorted;
        std::vector<std::pair<int32_t, int32_t>> by_id;
        for (int i = lo; i < hi; ++i) {
            const Analyzed &a = docs[i];
            auto &out = pairs[i];
            dl[i] = (int32_t)a.ids.size();
            if (want_positions) {   // (id, position) sorted: the positions of each id ascending, ids as the pairs below
                by_id.clear();
                for (size_t t = 0; t < a.ids.size(); ++t)
                    if (a.ids[t] >= 0) by_id.emplace_back(a.ids[t], (int32_t)t);
                std::sort(by_id.begin(), by_id.end());
                where[i].reserve(by_id.size());
                for (const auto &ip : by_id) where[i].push_back(ip.second);
            }
            sorted.clear();
            for (int32_t id : a.ids)
                if (id >= 0) sorted.push_back(id);
            std::sort(sorted.begin(), sorted.end());
            for (size_t j = 0; j < sorted.size();) {
                size_t e = j;
                while (e < sorted.size() && sorted[e] == sorted[j]) ++e;
                out.emplace_back(sorted[j], (int32_t)(e - j));
                j = e;
            }
            if (mode == MMRAG_LEX_QUERIES) {
                // first-occurrence order: rank each distinct id by the position it first appears at
                std::vector<std::pair<size_t, std::pair<int32_t, int32_t>>> first;
                for (const auto &p : out) {
                    const size_t at = (size_t)(std::find(a.ids.begin(), a.ids.end(), p.first) - a.ids.begin());
                    first.emplace_back(at, p);
                }
                std::sort(first.begin(), first.end());
                for (size_t j = 0; j < out.size(); ++j) out[j] = first[j].second;
            }
        }
    });
    out_offsets[0] = 0;
    for (int i = 0; i < n; ++i) out_offsets[i + 1] = out_offsets[i] + (int64_t)pairs[i].size();
    std::vector<int64_t> pos_at((size_t)(want_positions ? n + 1 : 0), 0);
    if (want_positions) {
        for (int i = 0; i < n; ++i) pos_at[i + 1] = pos_at[i] + (int64_t)where[i].size();
        *pos_needed = pos_at[n];
    }
    if (out_offsets[n] > capacity) {
        set_error("%s: %lld pairs > capacity %lld", name, (long long)out_offsets[n], (long long)capacity);
        return MMRAG_EWORKSPACE;
    }
    if (want_positions && pos_at[n] > pos_capacity) {
        set_error("%s: %lld positions > capacity %lld", name, (long long)pos_at[n], (long long)pos_capacity);
        return MMRAG_EWORKSPACE;
    }
    parallel_slices(n, n_threads, [&](int lo, int hi) {
        for (int i = lo; i < hi; ++i) {
            int64_t at = out_offsets[i];
            for (const auto &p : pairs[i]) {
                term_ids[at] = p.first;
                tfs[at++] = p.second;
            }
            if (want_positions && !where[i].empty())
                memcpy(positions + pos_at[i], where[i].data(), where[i].size() * sizeof(int32_t));
        }
    });
    return MMRAG_OK;
}

int mmrag_lexicon_analyze_batch(void *lexicon, const uint32_t *cps, const int64_t *offsets, int n, int mode,
                                int64_t *out_offsets, int32_t *term_ids, int32_t *tfs, int32_t *dl, int64_t capacity,
                                int n_threads) {
    return analyze_batch_impl("lexicon_analyze_batch", lexicon, cps, offsets, n, mode, out_offsets, term_ids, tfs, dl,
                              capacity, false, nullptr, 0, nullptr, n_threads);
}

// mmrag_lexicon_analyze_batch in MMRAG_LEX_DOCUMENTS mode plus where in its text every pair's term stands
int mmrag_lexicon_analyze_positions(void *lexicon, const uint32_t *cps, const int64_t *offsets, int n,
                                    int64_t *out_offsets, int32_t *term_ids, int32_t *tfs, int32_t *dl,
                                    int64_t capacity, int32_t *positions, int64_t pos_capacity, int64_t *pos_needed,
                                    int n_threads) {
    return analyze_batch_impl("lexicon_analyze_positions", lexicon, cps, offsets, n, MMRAG_LEX_DOCUMENTS, out_offsets,
                              term_ids, tfs, dl, capacity, true, positions, pos_capacity, pos_needed, n_threads);
}

// Terms first_id .. first_id + count as code points: the pool is in id order, so the answer is one slice of it.
int mmrag_lexicon_export(const void *lexicon, int32_t first_id, int32_t count, int64_t *offsets, uint32_t *cps,
                         int64_t capacity) {
    MMRAG_CHECK_ARG(lexicon && offsets, "lexicon_export: null pointer");
    const Lexicon &lx = *(const Lexicon *)lexicon;
    MMRAG_CHECK_ARG(first_id >= 0 && count >= 0 && (int64_t)first_id + count <= lx.n,
                    "lexicon_export: terms %d .. %lld outside the lexicon's %d", first_id, (long long)first_id + count, lx.n);
    MMRAG_CHECK_ARG(capacity >= 0, "lexicon_export: capacity=%lld", (long long)capacity);
    auto start_of = [&](int64_t id) { return id < lx.n ? lx.starts[(size_t)id] : (uint64_t)lx.pool.size(); };
    const uint64_t base = start_of(first_id);
    for (int32_t i = 0; i <= count; ++i) offsets[i] = (int64_t)(start_of((int64_t)first_id + i) - base);
    if (offsets[count] > capacity) {
        set_error("lexicon_export: %lld code points > capacity %lld", (long long)offsets[count], (long long)capacity);
        return MMRAG_EWORKSPACE;
    }
    MMRAG_CHECK_ARG(offsets[count] == 0 || cps, "lexicon_export: null output");
    if (offsets[count]) memcpy(cps, &lx.pool[base], (size_t)offsets[count] * 4);
    return MMRAG_OK;
}

// The query mode that keeps unknown terms: every distinct term of each text in order of first occurrence, with its id
// (-1: not in the lexicon) and its code points.  Threads as mmrag_lexicon_analyze_batch; nothing is inserted.
int mmrag_lexicon_analyze_terms(const void *lexicon, const uint32_t *cps, const int64_t *offsets, int n,
                                int64_t *out_offsets, int32_t *term_ids, int64_t *cp_offsets, uint32_t *out_cps,
                                int64_t term_capacity, int64_t cp_capacity, int64_t *needed, int n_threads) {
    MMRAG_CHECK_ARG(lexicon && offsets && out_offsets && needed, "lexicon_analyze_terms: null pointer");
    MMRAG_CHECK_ARG(n >= 0, "lexicon_analyze_terms: n=%d", n);
    MMRAG_CHECK_ARG(n == 0 || cps || offsets[n] == offsets[0], "lexicon_analyze_terms: null text");
    MMRAG_CHECK_ARG(term_capacity >= 0 && cp_capacity >= 0 && cp_offsets &&
                        (term_capacity == 0 || term_ids) && (cp_capacity == 0 || out_cps),
                    "lexicon_analyze_terms: null output");
    const Lexicon &lx = *(const Lexicon *)lexicon;
    if (n_threads < 1) n_threads = 1;
    if (n > 0) {
        const int64_t by_work = 1 + (offsets[n] - offsets[0]) / 16384;
        if (n_threads > by_work) n_threads = (int)by_work;
    }
    // per text: the distinct terms as (begin, end) in its own pool, and their ids
    struct Distinct {
        Analyzed a;
        std::vector<std::pair<uint32_t, uint32_t>> spans;
        std::vector<int32_t> ids;
        int64_t n_cps = 0;
    };
    std::vector<Distinct> docs((size_t)n);
    parallel_slices(n, n_threads, [&](int lo, int hi) {
        for (int i = lo; i < hi; ++i) {
            Distinct &d = docs[i];
            analyze_text(cps + offsets[i], (size_t)(offsets[i + 1] - offsets[i]), d.a);
            for (size_t t = 0, b = 0; t < d.a.ends.size(); b = d.a.ends[t++]) {
                const uint32_t e = d.a.ends[t];
                bool seen = false;
                for (const auto &s : d.spans)
                    if (s.second - s.first == e - b && !memcmp(&d.a.pool[s.first], &d.a.pool[b], (size_t)(e - b) * 4)) {
                        seen = true;
                        break;
                    }
                if (seen) continue;
                d.spans.emplace_back((uint32_t)b, e);
                d.ids.push_back(lx.find(&d.a.pool[b], e - b));
                d.n_cps += e - b;
            }
        }
    });
    out_offsets[0] = 0;
    std::vector<int64_t> cp_at((size_t)n + 1, 0);
    for (int i = 0; i < n; ++i) {
        out_offsets[i + 1] = out_offsets[i] + (int64_t)docs[i].ids.size();
        cp_at[i + 1] = cp_at[i] + docs[i].n_cps;
    }
    needed[0] = out_offsets[n];
    needed[1] = cp_at[n];
    if (needed[0] > term_capacity || needed[1] > cp_capacity) {
        set_error("lexicon_analyze_terms: %lld terms, %lld code points > capacity %lld, %lld", (long long)needed[0],
                  (long long)needed[1], (long long)term_capacity, (long long)cp_capacity);
        return MMRAG_EWORKSPACE;
    }
    cp_offsets[0] = 0;
    parallel_slices(n, n_threads, [&](int lo, int hi) {
        for (int i = lo; i < hi; ++i) {
            const Distinct &d = docs[i];
            int64_t at = out_offsets[i], cp = cp_at[i];
            for (size_t t = 0; t < d.ids.size(); ++t, ++at) {
                const uint32_t len = d.spans[t].second - d.spans[t].first;
                term_ids[at] = d.ids[t];
                if (len) memcpy(out_cps + cp, &d.a.pool[d.spans[t].first], (size_t)len * 4);
                cp += len;
                cp_offsets[at + 1] = cp;
            }
        }
    });
    return MMRAG_OK;
}

}  // extern "C"
