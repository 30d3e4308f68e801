// Stand-alone check of the pure plans of the operators over raw samples: the sample conditioner's (csrc/gat_cond_plan.h), the
// sample beamformer's (csrc/gat_beam_plan.h) and the pieces they share (csrc/gat_sig_plan.h), over a few thousand random cases
// each.  Every planned call must cover each (block, sample) exactly once through the units the kernels walk, dealt to the grid
// exactly once, with the streaming kernel chosen exactly under its rule; every documented refusal must return its code with
// nothing planned.  (The estimating operators' split and batches: tests/estplan.)  Built with -fsanitize=address,undefined by
// tests/test_condition_plan_host.py.  No memory behind the descriptors is ever touched: the plans read addresses, not data.
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "gat_beam_plan.h"
#include "gat_cond_plan.h"

using namespace gat;

namespace {

int failures = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            if (++failures <= 20) {                       \
                std::printf("FAIL %s:%d: ", #cond, __LINE__); \
                std::printf(__VA_ARGS__);                 \
                std::printf("\n");                        \
            }                                             \
        }                                                 \
    } while (0)

const CondPlan kUntouched = {true, true, -7, -7, -7, -7, -7};
template <class Plan> // (field by field: the structs have padding)
bool split_untouched(const Plan &p) { return p.stream && p.group == -7 && p.chunk == -7 && p.chunks == -7 && p.units == -7 && p.grid == -7; }
bool untouched(const CondPlan &p) { return split_untouched(p) && p.in_place; }

gat_signal_desc desc(uintptr_t re, uintptr_t im, int layout, int M, long long N, long long as, long long bs)
{
    gat_signal_desc d{};
    d.re = reinterpret_cast<const void *>(re);
    d.im = layout == GAT_LAYOUT_PLANAR ? reinterpret_cast<const void *>(im) : nullptr;
    d.layout = layout;
    d.num_ants = M;
    d.num_samples = N;
    d.ant_stride = as;
    d.block_stride = bs;
    d.chan_stride = 0;
    return d;
}

void expect_refusal(const gat_signal_desc *s, int B, const void *prm, uint32_t flags, const gat_signal_desc *o, int code, const char *what)
{
    CondPlan p = kUntouched;
    const Refusal r = cond_plan(s, B, prm, flags, o, 2048, &p);
    CHECK(r.code == code, "%s: got %d, want %d", what, r.code, code);
    CHECK(r.code == GAT_OK || r.msg != nullptr, "%s: a refusal without a message", what);
    CHECK(untouched(p), "%s: a refused call planned something", what);
}

// walks a (block, chunk) plan -- the conditioner's or the beamformer's: their kernels decode a unit alike -- as the kernels do
// and counts every (block, sample); group: what a lane of the streaming kernel owns per step
template <class Plan>
void check_cover(const Plan &p, int B, long long N, int group)
{
    std::vector<unsigned char> hits((size_t)B * (size_t)N, 0);
    std::vector<unsigned char> dealt((size_t)p.units, 0);
    CHECK(p.grid >= 1 && p.grid <= p.units, "grid %lld of %lld units", p.grid, p.units);
    CHECK(p.units == (long long)B * p.chunks && p.units < (1ll << 31), "units");
    CHECK(p.group == (p.stream ? group : 1), "group %d", p.group);
    CHECK(p.chunk % ((long long)kCondThreads * p.group) == 0 && p.chunk > 0, "chunk %lld", p.chunk);
    for (long long g = 0; g < p.grid; ++g)
        for (long long u = g; u < p.units; u += p.grid) {
            ++dealt[(size_t)u];
            long long b, n0, n1;
            cond_unit(u, p.chunks, p.chunk, N, &b, &n0, &n1);
            CHECK(b >= 0 && b < B && n0 >= 0 && n0 < n1 && n1 <= N, "unit %lld: block %lld samples [%lld, %lld)", u, b, n0, n1);
            if (!(b >= 0 && b < B && n0 >= 0 && n1 <= N)) continue;
            // the streaming kernel: whole groups by lane, then the block's ragged end one sample a lane
            const long long G = p.group, g1 = n1 / G;
            CHECK(n0 % G == 0, "a chunk starts inside a group");
            for (long long gi = n0 / G; gi < g1; ++gi)
                for (long long s = 0; s < G; ++s) ++hits[(size_t)(b * N + gi * G + s)];
            if (n1 == N)
                for (long long n = g1 * G; n < N; ++n) {
                    CHECK(n - g1 * G < kCondThreads, "the tail needs more lanes than a workgroup has");
                    ++hits[(size_t)(b * N + n)];
                }
            else
                CHECK(n1 % G == 0, "a chunk that is not the block's last ends inside a group");
        }
    for (size_t i = 0; i < dealt.size(); ++i) CHECK(dealt[i] == 1, "unit %zu dealt %d times", i, (int)dealt[i]);
    for (size_t i = 0; i < hits.size(); ++i)
        if (hits[i] != 1) {
            CHECK(false, "block %zu sample %zu covered %d times", i / (size_t)N, i % (size_t)N, (int)hits[i]);
            break;
        }
}

static_assert(kBeamThreads == kCondThreads, "check_cover's lane count is both kernels'");
const BeamPlan kBeamUntouched = {true, -7, -7, -7, -7, -7};
bool untouched(const BeamPlan &p) { return split_untouched(p); }
const double *const kWeights = reinterpret_cast<const double *>(uintptr_t(0x8000));

void expect_beam_refusal(const gat_signal_desc *s, int B, const double *w_re, const double *w_im, int J, const gat_signal_desc *o, int code,
                         const char *what)
{
    BeamPlan p = kBeamUntouched;
    const Refusal r = beam_plan(s, B, w_re, w_im, J, o, 2048, &p);
    CHECK(r.code == code, "beam, %s: got %d, want %d", what, r.code, code);
    CHECK(r.code == GAT_OK || r.msg != nullptr, "beam, %s: a refusal without a message", what);
    CHECK(untouched(p), "beam, %s: a refused call planned something", what);
}

// gat_beamform_samples: random (signal, output) pairs; returns the calls that streamed
int sweep_beam_plans(std::mt19937_64 &rng)
{
    auto pick = [&](long long lo, long long hi) { return (long long)(rng() % (uint64_t)(hi - lo + 1)) + lo; };
    int planned = 0, streamed = 0;
    for (int it = 0; it < 3000; ++it) {
        const int li = (int)pick(0, 3), lo = (int)pick(0, 1);
        const int M = (int)(it % 5 == 0 ? pick(1, 64) : pick(1, 9)), J = (int)(it % 6 == 0 ? pick(1, 64) : pick(1, 5));
        const int B = (int)(it % 7 == 0 ? pick(1, 300) : pick(1, 4));
        const long long N = it % 11 == 0 ? pick(1, 300000) / B + 1 : pick(1, 3000);
        const bool tidy = it % 2 == 0;
        const long long vi = layout_vec_samples(li), vo = layout_vec_samples(lo);
        const long long ibs = tidy ? (N + vi - 1) / vi * vi : N + pick(0, 9), obs = tidy ? (N + vo - 1) / vo * vo : N + pick(0, 9);
        const long long ias = ibs * B + (tidy ? vi * pick(0, 3) : pick(0, 5)), oas = obs * B + (tidy ? vo * pick(0, 3) : pick(0, 5));
        const uintptr_t ioff = tidy ? 0 : (uintptr_t)pick(0, 3) * layout_sample_bytes(li), ooff = tidy ? 0 : (uintptr_t)pick(0, 3) * layout_sample_bytes(lo);
        const gat_signal_desc s = desc(0x100000000ull + ioff, 0x200000000ull + ioff, li, M, N, ias, ibs);
        const gat_signal_desc o = desc(0x300000000ull + ooff, 0x400000000ull + ooff, lo, J, N, oas, obs);
        const long long want = pick(1, 3) == 1 ? pick(1, 64) : 2048;
        BeamPlan p = kBeamUntouched;
        const Refusal r = beam_plan(&s, B, kWeights, kWeights, J, &o, want, &p);
        CHECK(r.code == GAT_OK, "beam: a valid call was refused: %d %s", r.code, r.msg ? r.msg : "");
        if (r.code != GAT_OK) continue;
        ++planned;
        const bool rule = M <= kBeamStreamMaxAnts && blocks_aligned(&s, B) && blocks_aligned(&o, B);
        CHECK(p.stream == rule, "beam: stream %d, the rule says %d", (int)p.stream, (int)rule);
        CHECK(!tidy || M > kBeamStreamMaxAnts || p.stream, "beam: an aligned call did not stream");
        streamed += p.stream;
        if ((long long)B * N <= 400000) check_cover(p, B, N, beam_group_samples(li));

        // the refusals, each from this valid pair
        gat_signal_desc t = s, v = o;
        expect_beam_refusal(nullptr, B, kWeights, kWeights, J, &o, GAT_ERR_ARG, "null signal");
        expect_beam_refusal(&s, B, kWeights, kWeights, J, nullptr, GAT_ERR_ARG, "null output");
        expect_beam_refusal(&s, B, nullptr, kWeights, J, &o, GAT_ERR_ARG, "null w_re");
        expect_beam_refusal(&s, B, kWeights, nullptr, J, &o, GAT_ERR_ARG, "null w_im");
        expect_beam_refusal(&s, 0, kWeights, kWeights, J, &o, GAT_ERR_ARG, "no blocks");
        v = o, v.num_ants = 0;
        expect_beam_refusal(&s, B, kWeights, kWeights, 0, &v, GAT_ERR_ARG, "no beams");
        t = s, t.layout = 4;
        expect_beam_refusal(&t, B, kWeights, kWeights, J, &o, GAT_ERR_ARG, "bad layout");
        t = s;
        t.im = li == GAT_LAYOUT_PLANAR ? nullptr : t.re;
        expect_beam_refusal(&t, B, kWeights, kWeights, J, &o, GAT_ERR_ARG, "signal planes");
        t = s, t.re = nullptr;
        expect_beam_refusal(&t, B, kWeights, kWeights, J, &o, GAT_ERR_ARG, "no signal plane");
        t = s, t.num_samples = 0;
        expect_beam_refusal(&t, B, kWeights, kWeights, J, &o, GAT_ERR_ARG, "no samples");
        t = s, t.num_ants = 0;
        expect_beam_refusal(&t, B, kWeights, kWeights, J, &o, GAT_ERR_ARG, "no antennas");
        t = s, t.ant_stride = -1;
        expect_beam_refusal(&t, B, kWeights, kWeights, J, &o, GAT_ERR_ARG, "negative ant_stride");
        t = s, t.block_stride = -1;
        expect_beam_refusal(&t, B, kWeights, kWeights, J, &o, GAT_ERR_ARG, "negative block_stride");
        v = o, v.ant_stride = -1;
        expect_beam_refusal(&s, B, kWeights, kWeights, J, &v, GAT_ERR_ARG, "negative output ant_stride");
        v = o, v.block_stride = -1;
        expect_beam_refusal(&s, B, kWeights, kWeights, J, &v, GAT_ERR_ARG, "negative output block_stride");
        t = s, t.num_ants = GAT_MAX_ARRAY_ANTS + 1;
        expect_beam_refusal(&t, B, kWeights, kWeights, J, &o, GAT_ERR_RANGE, "too many antennas");
        v = o, v.num_ants = GAT_MAX_ARRAY_ANTS + 1;
        expect_beam_refusal(&s, B, kWeights, kWeights, GAT_MAX_ARRAY_ANTS + 1, &v, GAT_ERR_RANGE, "too many beams");
        v = o, v.num_ants = J + 1;
        expect_beam_refusal(&s, B, kWeights, kWeights, J, &v, GAT_ERR_ARG, "num_ants is not num_beams");
        v = o, v.num_samples = N + 1;
        expect_beam_refusal(&s, B, kWeights, kWeights, J, &v, GAT_ERR_ARG, "num_samples mismatch");
        for (int l : {GAT_LAYOUT_INTERLEAVED_I16, GAT_LAYOUT_INTERLEAVED_I8}) {
            v = o, v.layout = l, v.im = nullptr;
            expect_beam_refusal(&s, B, kWeights, kWeights, J, &v, GAT_ERR_UNSUPPORTED, "an integer output");
        }
        v = o, v.layout = -1;
        expect_beam_refusal(&s, B, kWeights, kWeights, J, &v, GAT_ERR_ARG, "bad output layout");
        t = s, t.chan_stride = 8;
        expect_beam_refusal(&t, B, kWeights, kWeights, J, &o, GAT_ERR_UNSUPPORTED, "signal chan_stride");
        v = o, v.chan_stride = 8;
        expect_beam_refusal(&s, B, kWeights, kWeights, J, &v, GAT_ERR_UNSUPPORTED, "output chan_stride");
        v = o;
        v.im = lo == GAT_LAYOUT_PLANAR ? nullptr : v.re;
        expect_beam_refusal(&s, B, kWeights, kWeights, J, &v, GAT_ERR_ARG, "output planes");
        v = o, v.re = nullptr;
        expect_beam_refusal(&s, B, kWeights, kWeights, J, &v, GAT_ERR_ARG, "no output plane");
        if (M > 1) {
            t = s, t.ant_stride = 0;
            expect_beam_refusal(&t, B, kWeights, kWeights, J, &o, GAT_ERR_ARG, "zero ant_stride");
            t = s, t.ant_stride = 1ll << 60;
            expect_beam_refusal(&t, B, kWeights, kWeights, J, &o, GAT_ERR_RANGE, "signal extent");
        }
        if (B > 1) {
            t = s, t.block_stride = 0;
            expect_beam_refusal(&t, B, kWeights, kWeights, J, &o, GAT_ERR_ARG, "zero block_stride");
            v = o, v.block_stride = 0;
            expect_beam_refusal(&s, B, kWeights, kWeights, J, &v, GAT_ERR_ARG, "zero output block_stride");
        }
        if (J > 1) {
            v = o, v.ant_stride = 0;
            expect_beam_refusal(&s, B, kWeights, kWeights, J, &v, GAT_ERR_ARG, "zero output ant_stride");
            v = o, v.ant_stride = 1ll << 60;
            expect_beam_refusal(&s, B, kWeights, kWeights, J, &v, GAT_ERR_RANGE, "output extent");
        }
        // overlap: the output starts on the last byte of either input plane, or either output plane is an input plane
        const uintptr_t in_bytes = (uintptr_t)((B - 1) * ibs + (M - 1) * ias + N) * layout_sample_bytes(li);
        v = o, v.re = reinterpret_cast<const void *>(reinterpret_cast<uintptr_t>(s.re) + in_bytes - 1);
        expect_beam_refusal(&s, B, kWeights, kWeights, J, &v, GAT_ERR_ARG, "the output starts on the input's last byte");
        if (li == GAT_LAYOUT_PLANAR) {
            v = o, v.re = reinterpret_cast<const void *>(reinterpret_cast<uintptr_t>(s.im) + in_bytes - 1);
            expect_beam_refusal(&s, B, kWeights, kWeights, J, &v, GAT_ERR_ARG, "the output starts on the last byte of the input's im plane");
        }
        if (lo == GAT_LAYOUT_PLANAR) {
            v = o, v.im = s.re;
            expect_beam_refusal(&s, B, kWeights, kWeights, J, &v, GAT_ERR_ARG, "the output's im plane is the input's re plane");
        }
        // an output that ends where the input begins is no overlap
        const uintptr_t out_bytes = (uintptr_t)((B - 1) * obs + (J - 1) * oas + N) * layout_sample_bytes(lo);
        if (lo != GAT_LAYOUT_PLANAR) {
            v = o, v.re = reinterpret_cast<const void *>(reinterpret_cast<uintptr_t>(s.re) - out_bytes);
            BeamPlan z = kBeamUntouched;
            CHECK(beam_plan(&s, B, kWeights, kWeights, J, &v, want, &z).code == GAT_OK, "beam: an adjacent output was refused");
        }
    }
    std::printf("planned %d beam calls (%d streaming)\n", planned, streamed);
    CHECK(planned == 3000 && streamed > 700 && streamed < 2300, "the beam sweep lost its balance");
    return streamed;
}

} // namespace

int main()
{
    std::mt19937_64 rng(20261018);
    auto pick = [&](long long lo, long long hi) { return (long long)(rng() % (uint64_t)(hi - lo + 1)) + lo; };
    const gat_cond_params *prm = reinterpret_cast<const gat_cond_params *>(uintptr_t(0x7000));
    int planned = 0, streamed = 0, in_place = 0;

    for (int it = 0; it < 4000; ++it) {
        const int li = (int)pick(0, 3), lo = (int)pick(0, 3);
        const int M = (int)(it % 5 == 0 ? pick(1, 64) : pick(1, 9)), B = (int)(it % 7 == 0 ? pick(1, 300) : pick(1, 4));
        const long long N = it % 11 == 0 ? pick(1, 300000) / B + 1 : pick(1, 3000);
        const bool tidy = it % 2 == 0; // aligned bases and strides: the streaming kernel's candidates
        const long long vi = layout_vec_samples(li), vo = layout_vec_samples(lo);
        const long long ibs = tidy ? (N + vi - 1) / vi * vi : N + pick(0, 9), obs = tidy ? (N + vo - 1) / vo * vo : N + pick(0, 9);
        const long long ias = ibs * B + (tidy ? vi * pick(0, 3) : pick(0, 5)), oas = obs * B + (tidy ? vo * pick(0, 3) : pick(0, 5));
        const uintptr_t ioff = tidy ? 0 : (uintptr_t)pick(0, 3) * layout_sample_bytes(li), ooff = tidy ? 0 : (uintptr_t)pick(0, 3) * layout_sample_bytes(lo);
        // four regions far apart: input planes, output planes
        const gat_signal_desc s = desc(0x100000000ull + ioff, 0x200000000ull + ioff, li, M, N, ias, ibs);
        const gat_signal_desc o = desc(0x300000000ull + ooff, 0x400000000ull + ooff, lo, M, N, oas, obs);
        const long long want = pick(1, 3) == 1 ? pick(1, 64) : 2048;
        CondPlan p = kUntouched;
        const Refusal r = cond_plan(&s, B, prm, (uint32_t)pick(0, 1), &o, want, &p);
        CHECK(r.code == GAT_OK, "a valid call was refused: %d %s", r.code, r.msg ? r.msg : "");
        if (r.code != GAT_OK) continue;
        ++planned;
        const bool rule = M <= kCondStreamMaxAnts && blocks_aligned(&s, B) && blocks_aligned(&o, B);
        CHECK(p.stream == rule, "stream %d, the rule says %d", (int)p.stream, (int)rule);
        CHECK(!tidy || M > kCondStreamMaxAnts || p.stream, "an aligned call did not stream");
        CHECK(!p.in_place, "in_place without identical descriptors");
        streamed += p.stream;
        if ((long long)B * N <= 400000) check_cover(p, B, N, cond_group_samples(li, lo));

        // in place: the same descriptor on both sides
        CondPlan q = kUntouched;
        const Refusal r2 = cond_plan(&s, B, prm, 0, &s, want, &q);
        CHECK(r2.code == GAT_OK && q.in_place, "in place refused: %d", r2.code);
        in_place += r2.code == GAT_OK;

        // the refusals, each from this valid pair
        gat_signal_desc t = s, v = o;
        expect_refusal(nullptr, B, prm, 0, &o, GAT_ERR_ARG, "null signal");
        expect_refusal(&s, B, prm, 0, nullptr, GAT_ERR_ARG, "null output");
        expect_refusal(&s, B, nullptr, 0, &o, GAT_ERR_ARG, "null records");
        expect_refusal(&s, 0, prm, 0, &o, GAT_ERR_ARG, "no blocks");
        expect_refusal(&s, B, prm, 2u, &o, GAT_ERR_ARG, "unknown flag");
        t = s, t.num_samples = 0;
        expect_refusal(&t, B, prm, 0, &o, GAT_ERR_ARG, "no samples");
        t = s, t.num_ants = 0;
        expect_refusal(&t, B, prm, 0, &o, GAT_ERR_ARG, "no antennas");
        t = s, t.ant_stride = -1;
        expect_refusal(&t, B, prm, 0, &o, GAT_ERR_ARG, "negative ant_stride");
        v = o, v.block_stride = -1;
        expect_refusal(&s, B, prm, 0, &v, GAT_ERR_ARG, "negative output block_stride");
        if (M > 1) {
            v = o, v.ant_stride = 0;
            expect_refusal(&s, B, prm, 0, &v, GAT_ERR_ARG, "zero output ant_stride");
        }
        if (B > 1) {
            t = s, t.block_stride = 0;
            expect_refusal(&t, B, prm, 0, &o, GAT_ERR_ARG, "zero block_stride");
        }
        v = o, v.num_ants = M + 1;
        expect_refusal(&s, B, prm, 0, &v, GAT_ERR_ARG, "num_ants mismatch");
        v = o, v.num_samples = N + 1;
        expect_refusal(&s, B, prm, 0, &v, GAT_ERR_ARG, "num_samples mismatch");
        t = s, t.layout = 4;
        expect_refusal(&t, B, prm, 0, &o, GAT_ERR_ARG, "bad layout");
        v = o, v.layout = -1;
        expect_refusal(&s, B, prm, 0, &v, GAT_ERR_ARG, "bad output layout");
        t = s;
        t.im = li == GAT_LAYOUT_PLANAR ? nullptr : t.re; // planar without im, interleaved with im
        expect_refusal(&t, B, prm, 0, &o, GAT_ERR_ARG, "signal planes");
        v = o;
        v.im = lo == GAT_LAYOUT_PLANAR ? nullptr : v.re;
        expect_refusal(&s, B, prm, 0, &v, GAT_ERR_ARG, "output planes");
        t = s, t.chan_stride = 8;
        expect_refusal(&t, B, prm, 0, &o, GAT_ERR_UNSUPPORTED, "signal chan_stride");
        v = o, v.chan_stride = 8;
        expect_refusal(&s, B, prm, 0, &v, GAT_ERR_UNSUPPORTED, "output chan_stride");
        t = s, v = o, t.num_ants = v.num_ants = GAT_MAX_ARRAY_ANTS + 1;
        expect_refusal(&t, B, prm, 0, &v, GAT_ERR_RANGE, "too many antennas");
        t = s, t.ant_stride = 1ll << 60;
        if (M > 1) expect_refusal(&t, B, prm, 0, &o, GAT_ERR_RANGE, "extent");
        // overlap: the output starts inside the input's extent (its last byte, or one sample in), in every plane pairing
        const uintptr_t in_bytes = (uintptr_t)((B - 1) * ibs + (M - 1) * ias + N) * layout_sample_bytes(li);
        v = o, v.re = reinterpret_cast<const void *>(reinterpret_cast<uintptr_t>(s.re) + in_bytes - 1);
        expect_refusal(&s, B, prm, 0, &v, GAT_ERR_ARG, "the output starts on the input's last byte");
        if (lo == GAT_LAYOUT_PLANAR) {
            v = o, v.im = s.re;
            expect_refusal(&s, B, prm, 0, &v, GAT_ERR_ARG, "the output's im plane is the input's re plane");
        }
        if (li == GAT_LAYOUT_PLANAR) {
            v = o, v.re = reinterpret_cast<const void *>(reinterpret_cast<uintptr_t>(s.im) + layout_sample_bytes(li));
            expect_refusal(&s, B, prm, 0, &v, GAT_ERR_ARG, "the output starts inside the input's im plane");
        }
        // the same memory, not the same elements
        t = s;
        t.re = reinterpret_cast<const void *>(reinterpret_cast<uintptr_t>(s.re) + layout_sample_bytes(li));
        expect_refusal(&s, B, prm, 0, &t, GAT_ERR_ARG, "in place, one sample on");
        if (B > 1) {
            t = s, t.block_stride = ibs + 1;
            expect_refusal(&s, B, prm, 0, &t, GAT_ERR_ARG, "in place with another block_stride");
        }
        // an output that ends where the input begins is no overlap
        const uintptr_t out_bytes = (uintptr_t)((B - 1) * obs + (M - 1) * oas + N) * layout_sample_bytes(lo);
        if (lo != GAT_LAYOUT_PLANAR) {
            v = o, v.re = reinterpret_cast<const void *>(reinterpret_cast<uintptr_t>(s.re) - out_bytes);
            CondPlan z = kUntouched;
            CHECK(cond_plan(&s, B, prm, 0, &v, want, &z).code == GAT_OK, "an adjacent output was refused");
        }
    }
    CHECK(planned == 4000 && streamed > 1000 && streamed < 3000, "the sweep lost its balance");
    sweep_beam_plans(rng);
    std::printf("planned %d calls (%d streaming, %d in place), %d failures\n", planned, streamed, in_place, failures);
    return failures ? 1 : 0;
}
