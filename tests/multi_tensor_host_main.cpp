// The host half of regtr_amd/csrc/multi_tensor.h alone, as a program of its own (tests/test_multi_tensor_host.py builds it with the host
// compiler under -fsanitize=address,undefined and runs it): mt_walk with a `launch` that only records and checks the chunks.
//   multi_tensor_host_main CAP(40|48) SLICE(4096|8192) KEEP_EMPTY(0|1)  ->  "<cases> cases, <chunks> chunks ok", exit status 0
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "multi_tensor.h"

struct Entry {
    long long n;
    int tensor;
    int wg0;
};

static int g_chunks = 0;

#define CHECK(cond)                                                                                  \
    do {                                                                                             \
        if (!(cond)) {                                                                               \
            std::printf("case %s: `%s` does not hold (line %d)\n", name, #cond, __LINE__);           \
            std::exit(1);                                                                            \
        }                                                                                            \
    } while (0)

// one walk over `lens`; every chunk is checked where it is launched, the whole call afterwards.  -> the number of chunks
template <int CAP, int SLICE>
int run_case(const char* name, const std::vector<long long>& lens, bool keep_empty)
{
    typedef MtChunk<Entry, CAP> Chunk;
    auto wgs_of = [&](int i) { return (lens[i] + SLICE - 1) / SLICE; };
    std::vector<int> seen;                                                     // the tensors of all entries, in launch order
    long long total = 0;                                                       // workgroups launched so far
    int chunks = 0;
    const int st = mt_walk<Chunk>(
        (int)lens.size(), keep_empty, wgs_of, [&](int i, Entry& e) { e.n = lens[i]; e.tensor = i; e.wg0 = -12345; },
        [&](const Chunk& c) {
            CHECK(c.n_entries >= 1 && c.n_entries <= CAP);
            CHECK(c.part0 == total);
            long long prefix = 0;
            for (int j = 0; j < c.n_entries; j++) {
                const Entry& e = c.e[j];
                const long long wgs = wgs_of(e.tensor);
                CHECK(e.n == lens[e.tensor]);
                CHECK(keep_empty || wgs > 0);
                CHECK(e.wg0 == prefix);                                        // the exclusive prefix of the entries' workgroups
                prefix += wgs;
                CHECK(prefix <= MT_MAX_WG);
                seen.push_back(e.tensor);
            }
            CHECK(c.n_wg == prefix);
            CHECK(keep_empty || c.n_wg > 0);
            // the search: the first, a middle and the last block of every entry find that entry -- so an entry WITHOUT a workgroup is
            // never the last one with wg0 <= b -- and the slices tile [0, n)
            for (int j = 0; j < c.n_entries; j++) {
                const Entry& e = c.e[j];
                const long long wgs = wgs_of(e.tensor);
                if (wgs == 0) continue;
                const long long blocks[3] = {e.wg0, e.wg0 + wgs / 2, e.wg0 + wgs - 1};
                for (long long b : blocks) {
                    CHECK(mt_search(c, (int)b) == j);
                    long long lo, hi;
                    mt_slice<SLICE>((int)b, e, lo, hi);
                    CHECK(lo == (b - e.wg0) * SLICE && lo < hi && hi - lo <= SLICE && hi <= e.n);
                    CHECK((b == e.wg0 + wgs - 1) == (hi == e.n));
                }
            }
            total += c.n_wg;
            chunks++;
            return 0;
        });
    CHECK(st == 0);
    // over the whole call: the entries are the tensors that were not skipped, in order
    std::vector<int> want;
    long long want_total = 0;
    for (int i = 0; i < (int)lens.size(); i++) {
        if (keep_empty || wgs_of(i) > 0) want.push_back(i);
        want_total += wgs_of(i);
    }
    CHECK(seen == want);
    CHECK(total == want_total);
    CHECK(chunks >= (int)((want.size() + CAP - 1) / CAP));
    g_chunks += chunks;
    return chunks;
}

static std::vector<long long> many(int n)
{
    std::vector<long long> v;
    for (int i = 0; i < n; i++) v.push_back(1 + i % 5);
    return v;
}

template <int CAP, int SLICE>
int run_all(bool keep)
{
    const char* name = "counts";
    int cases = 0;
    auto run = [&](const char* nm, const std::vector<long long>& lens) { cases++; return run_case<CAP, SLICE>(nm, lens, keep); };
    CHECK(run("no tensor", {}) == 0);
    CHECK(run("one tensor", {5}) == 1);
    CHECK(run("CAP - 1", many(CAP - 1)) == 1);
    CHECK(run("CAP", many(CAP)) == 1);
    CHECK(run("CAP + 1", many(CAP + 1)) == 2);
    CHECK(run("2 CAP + 1", many(2 * CAP + 1)) == 3);
    CHECK(run("slice - 1, slice, slice + 1", {SLICE - 1, SLICE, SLICE + 1}) == 1);
    // empty tensors: at the start, in the middle, at the end, alone, and as a whole chunk
    CHECK(run("empty at the start", {0, 0, 3, 7}) == 1);
    CHECK(run("empty in the middle", {3, 0, 0, 7}) == 1);
    CHECK(run("empty at the end", {3, 7, 0, 0}) == 1);
    CHECK(run("only empty", {0, 0, 0}) == (keep ? 1 : 0));
    {
        std::vector<long long> lens = {3, 9};
        lens.insert(lens.end(), CAP, 0);                                       // kept: they fill the rest of chunk 0 and start chunk 1
        lens.push_back(SLICE + 1);
        lens.push_back(0);
        CHECK(run("CAP empty ones", lens) == (keep ? 2 : 1));
        std::vector<long long> whole(CAP, 1);                                  // chunk 0 full, then CAP empty ones: a chunk without a workgroup
        whole.insert(whole.end(), CAP, 0);
        whole.push_back(2);
        CHECK(run("a whole chunk of empty ones", whole) == (keep ? 3 : 2));
    }
    // the flush no launch on a device can reach: workgroup counts that sum past 2^31 - 1, lengths up to 2^40 - 1 (the largest accepted)
    const long long big = (1ll << 40) - 1, big_wgs = (big + SLICE - 1) / SLICE, per = MT_MAX_WG / big_wgs;
    CHECK(per >= 1 && per < CAP);
    CHECK(run("35 of 2^40 - 1", std::vector<long long>(35, big)) == (int)((35 + per - 1) / per));
    {
        std::vector<long long> lens;                                           // empty ones between the large ones
        for (int i = 0; i < 20; i++) { lens.push_back(big); lens.push_back(0); }
        const int chunks = run("2^40 - 1 and empty ones", lens);
        CHECK(chunks >= (int)((20 + per - 1) / per));
    }
    {
        std::vector<long long> lens(per, big);                                 // per * big_wgs workgroups, then exactly the rest of 2^31 - 1
        const long long rest = MT_MAX_WG - per * big_wgs;
        if (rest > 0) lens.push_back(rest * SLICE);
        CHECK(run("exactly 2^31 - 1", lens) == 1);
        lens.push_back(1);                                                     // one workgroup more: a second launch
        CHECK(run("2^31", lens) == 2);
    }
    // a launch that fails ends the walk with its status
    {
        int calls = 0;
        const std::vector<long long> lens = many(2 * CAP + 1);
        const int st = mt_walk<MtChunk<Entry, CAP>>(
            (int)lens.size(), keep, [&](int i) { return (lens[i] + SLICE - 1) / SLICE; }, [&](int i, Entry& e) { e.n = lens[i]; e.tensor = i; },
            [&](const MtChunk<Entry, CAP>&) { return ++calls == 2 ? -1 : 0; });
        CHECK(st == -1 && calls == 2);
        cases++;
    }
    return cases;
}

int main(int argc, char** argv)
{
    if (argc != 4) {
        std::printf("usage: %s CAP SLICE KEEP_EMPTY\n", argv[0]);
        return 2;
    }
    const int cap = std::atoi(argv[1]), slice = std::atoi(argv[2]);
    const bool keep = std::atoi(argv[3]) != 0;
    int cases = -1;
    if (cap == 40 && slice == 4096) cases = run_all<40, 4096>(keep);
    else if (cap == 48 && slice == 4096) cases = run_all<48, 4096>(keep);
    else if (cap == 48 && slice == 8192) cases = run_all<48, 8192>(keep);
    else if (cap == 40 && slice == 8192) cases = run_all<40, 8192>(keep);
    else return 2;
    std::printf("%d cases, %d chunks ok\n", cases, g_chunks);
    return 0;
}
