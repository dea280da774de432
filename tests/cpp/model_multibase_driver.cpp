// tests/cpp/model_multibase_driver.cpp -- the multi-base host model (pbccs_amd/csrc/arrow_model.cpp) on its own:
// RepeatMutationEnumerator, UniqueNearbyMutations, ApplyMutations and TargetToQueryPositions known answers of the
// reference's tests (TestMutationEnumerator.cpp:107-137, TestMutations.cpp:89-181).  No engine, no device: this
// is the program to build with host sanitizers.
#include <cstdio>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "arrow_model.hpp"

using pbccs::MutationEx;

static int failures = 0;
#define CHECK(x)                                                       \
    do {                                                               \
        if (!(x)) {                                                    \
            std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #x);    \
            ++failures;                                                \
        }                                                              \
    } while (0)

static MutationEx Mut(int type, int start, int end, const std::string& bases)
{
    MutationEx m;
    m.type = type;
    m.start = start;
    m.end = end;
    m.bases = bases;
    return m;
}

static std::set<MutationEx> Set(const std::vector<MutationEx>& v) { return std::set<MutationEx>(v.begin(), v.end()); }

int main()
{
    {
        std::vector<MutationEx> got;
        pbccs::repeat_mutations("ACACACGCGCGTGTG", 2, 3, 0, 15, &got);
        CHECK(got.size() == 4);
        CHECK(Set(got) == Set({Mut(0, 0, 0, "AC"), Mut(1, 0, 2, ""), Mut(0, 5, 5, "CG"), Mut(1, 5, 7, "")}));
    }
    {
        std::vector<MutationEx> got;
        pbccs::repeat_mutations("ACAACAACAGCAGCAGTAGTAG", 3, 3, 0, 22, &got);
        CHECK(got.size() == 4);
        CHECK(Set(got) == Set({Mut(0, 0, 0, "ACA"), Mut(1, 0, 3, ""), Mut(0, 7, 7, "CAG"), Mut(1, 7, 10, "")}));
    }
    {
        std::vector<MutationEx> got;
        pbccs::repeat_mutations("ACACACAC", 2, 0, 0, 8, &got);
        pbccs::repeat_mutations(std::string(200, 'A'), 32, 1, 0, 200, &got);
        CHECK(got.empty());
        pbccs::repeat_mutations("ACACACAC", 2, 3, -100, 100, &got);   // windows are clamped to the template
        CHECK(got.size() == 2);
        got.clear();
        pbccs::repeat_mutations("ACACACAC", 2, 3, 6, 8, &got);   // a window at the very end: no read past it
        CHECK(got.empty());
        pbccs::repeat_mutations(std::string(40, 'A'), 31, 1, 0, 40, &got);
        CHECK(!got.empty());
    }
    {
        std::vector<MutationEx> got;
        const std::string tpl = "TTACACACGGTTTGTGTGTGAA";
        pbccs::nearby_repeat_mutations(tpl, 2, 3, {3, 4, 14}, 3, &got);
        std::vector<MutationEx> all;
        pbccs::repeat_mutations(tpl, 2, 3, 0, (int)tpl.size(), &all);
        CHECK(Set(got) == Set(all));
        for (size_t k = 1; k < got.size(); ++k) CHECK(got[k - 1] < got[k]);
    }
    {
        std::string out;
        std::vector<int> mtp;
        CHECK(pbccs::apply_mutations_ex("GATTACA", {Mut(0, 3, 3, "C"), Mut(0, 2, 2, "T"), Mut(0, 0, 0, "G"),
                                                     Mut(2, 6, 7, "T"), Mut(1, 4, 5, "")}, &out, &mtp));
        CHECK(out == "GGATTCTCT");
        CHECK(pbccs::apply_mutations_ex("GATTACA", {Mut(2, 2, 3, "A"), Mut(0, 2, 2, "T")}, &out, &mtp));
        CHECK(out == "GATATACA");
        CHECK(pbccs::apply_mutations_ex("GATTACA", {Mut(1, 2, 3, ""), Mut(0, 5, 5, "C"), Mut(2, 4, 5, "G")}, &out, &mtp));
        CHECK((mtp == std::vector<int>{0, 1, 2, 2, 3, 5, 6, 7}));
        CHECK(pbccs::apply_mutations_ex("GG", {Mut(0, 0, 0, "A")}, &out, &mtp));
        CHECK((mtp == std::vector<int>{1, 2, 3}));
        CHECK(pbccs::apply_mutations_ex("AGG", {Mut(1, 0, 1, "")}, &out, &mtp));
        CHECK((mtp == std::vector<int>{0, 0, 1, 2}));
        // widths above one
        CHECK(pbccs::apply_mutations_ex("GATTACA", {Mut(0, 2, 2, "ACG"), Mut(1, 4, 6, ""), Mut(2, 0, 2, "TT")}, &out, &mtp));
        CHECK(out == "TTACGTTA");
        CHECK((mtp == std::vector<int>{0, 1, 5, 6, 7, 7, 7, 8}));
        CHECK(pbccs::apply_mutations_ex("GATTACA", {Mut(0, 7, 7, "AC")}, &out, &mtp));
        CHECK(out == "GATTACAAC");
        // refusals: outside the template, invalid, overlapping
        CHECK(!pbccs::apply_mutations_ex("GATTACA", {Mut(1, 5, 9, "")}, &out, &mtp));
        CHECK(!pbccs::apply_mutations_ex("GATTACA", {Mut(0, 8, 8, "A")}, &out, &mtp));
        CHECK(!pbccs::apply_mutations_ex("GATTACA", {Mut(2, 1, 4, "AC")}, &out, &mtp));
        CHECK(!pbccs::apply_mutations_ex("GATTACA", {Mut(0, 1, 2, "A")}, &out, &mtp));
        CHECK(!pbccs::apply_mutations_ex("GATTACA", {Mut(1, 1, 4, ""), Mut(2, 2, 4, "AC")}, &out, &mtp));
        CHECK(!pbccs::apply_mutations_ex("GATTACA", {Mut(1, -1, 2, "")}, &out, &mtp));
    }
    {
        // seeded random well-separated lists: lengths add up and the map is monotone
        std::mt19937 rng(7);
        for (int it = 0; it < 200; ++it) {
            const int L = 20 + (int)(rng() % 100);
            std::string t;
            for (int k = 0; k < L; ++k) t.push_back("ACGT"[rng() % 4]);
            std::vector<MutationEx> muts;
            int diff = 0;
            for (int p = (int)(rng() % 4); p + 8 < L; p += 5 + (int)(rng() % 9)) {
                const int kind = (int)(rng() % 3), w = 1 + (int)(rng() % 4);
                std::string b;
                for (int k = 0; k < w; ++k) b.push_back("ACGT"[rng() % 4]);
                muts.push_back(kind == 0 ? Mut(0, p, p, b) : kind == 1 ? Mut(1, p, p + w, "") : Mut(2, p, p + w, b));
                diff += muts.back().LengthDiff();
            }
            std::string out;
            std::vector<int> mtp;
            CHECK(pbccs::apply_mutations_ex(t, muts, &out, &mtp));
            CHECK((int)out.size() == L + diff);
            CHECK((int)mtp.size() == L + 1 && mtp[L] == (int)out.size());
            for (int k = 1; k <= L; ++k) CHECK(mtp[k - 1] <= mtp[k]);
            std::vector<MutationEx> rep;
            pbccs::repeat_mutations(t, 1 + (int)(rng() % 3), 2, (int)(rng() % L) - 5, (int)(rng() % L) + 5, &rep);
            for (const MutationEx& m : rep) CHECK(m.Valid() && m.start >= 0 && m.end <= L);
        }
    }
    std::printf(failures ? "failed %d\n" : "ok\n", failures);
    return failures ? 1 : 0;
}
