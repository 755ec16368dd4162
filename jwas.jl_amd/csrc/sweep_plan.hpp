// sweep_plan.hpp -- which schedule a sweep of a Float32 context takes: the JWAS_HIP_* switches (SweepKnobs), what the decision reads
// from the context and the parameters (SweepFacts), and the decision itself (plan_sweep: a pure function of the two).  Host code only
// and no HIP header: a host compiler compiles it alone (tests/test_sweep_plan_host.py evaluates it on a table of facts).
// jwas_hip.hip fills the facts, takes the plan and enqueues it; jwas_hip_last_sweep_schedule reports plan.sched plus the per-launch bits.
#pragma once
#include "../../include/jwas_hip.h"

#include <cstdint>
#include <cstdlib>

namespace jw {

// Every switch of the sweep's host side; -1 (a fraction: its default) = not set.
struct SweepKnobs {
    // read at every sweep (the tests flip them between sweeps of one process)
    int dense_mt = -1;              // JWAS_HIP_DENSE_MT=0|1: the dense-walk-only multi-trait instantiation off | on whatever the last sweep did
    bool dense_big_off = false;     // JWAS_HIP_DENSE_BIG_OFF (set): the same chain through the general path
    int compact_off = 0;            // JWAS_HIP_COMPACT_OFF=0..3: the speculative rounds instead of the compact chain
    int coop_apply = -1;            // JWAS_HIP_COOP_APPLY=0|1: the update role's cooperative apply (one block per launch)
    bool debug_phases = false;      // JWAS_HIP_DEBUG_PHASES (set): the sampler's counters on stderr after the sweep
    // read once per process (tests/test_gpu_schedule_variants.py runs every combination in a process of its own)
    double dense_mt_fraction = 0.1; // JWAS_HIP_DENSE_MT_FRACTION
    int corr_helper = 1;            // JWAS_HIP_CORR_HELPER=0: the next block's correction in the sampler, not in a helper workgroup
    int groups = 1;                 // JWAS_HIP_GROUPS=0: group_launch ignored
    int group_coop = -1;            // JWAS_HIP_GROUP_COOP=0|1
    int quiet_xcd = -1;             // JWAS_HIP_QUIET_XCD=0|1
    int pingpong = -1;              // JWAS_HIP_PINGPONG=0|1
    int debug_throttle = 0;         // JWAS_HIP_DEBUG_THROTTLE (builds with JWAS_HIP_DEV_KNOBS only)
};

inline SweepKnobs sweep_knobs()
{
    const auto num = [](const char* name, int unset) { const char* e = std::getenv(name); return e ? std::atoi(e) : unset; };
    static const SweepKnobs once = [&] {
        SweepKnobs k;
        if (const char* e = std::getenv("JWAS_HIP_DENSE_MT_FRACTION")) k.dense_mt_fraction = std::atof(e);
        k.corr_helper = num("JWAS_HIP_CORR_HELPER", 1);
        k.groups = num("JWAS_HIP_GROUPS", 1);
        k.group_coop = num("JWAS_HIP_GROUP_COOP", -1);
        k.quiet_xcd = num("JWAS_HIP_QUIET_XCD", -1);
        k.pingpong = num("JWAS_HIP_PINGPONG", -1);
#ifdef JWAS_HIP_DEV_KNOBS
        k.debug_throttle = num("JWAS_HIP_DEBUG_THROTTLE", 0);
#endif
        return k;
    }();
    SweepKnobs k = once;
    k.dense_mt = num("JWAS_HIP_DENSE_MT", -1);
    k.dense_big_off = std::getenv("JWAS_HIP_DENSE_BIG_OFF") != nullptr;
    k.compact_off = num("JWAS_HIP_COMPACT_OFF", 0);
    k.coop_apply = num("JWAS_HIP_COOP_APPLY", -1);
    k.debug_phases = std::getenv("JWAS_HIP_DEBUG_PHASES") != nullptr;
    return k;
}

// What the decision reads, as plain scalars.  multi_trait / sampler2: is_mt_method / is_sampler2 of kernels.hpp (the kernels' own
// predicates: that header is device code, so the caller evaluates them).
struct SweepFacts {
    int method = 0, t = 1;
    bool multi_trait = false, sampler2 = false;
    int64_t p = 0, nblocks = 0;
    int bs = 0;
    bool uniform = true;            // no explicit partition
    bool row_mode = false, packed = false;
    int gm = 0;                     // blocks per grouped launch of the selected block set (0: not set up)
    bool has_gpp = false, has_sync_cnt = false;
    double last_events = -1.0;      // effect changes of the previous sweep (-1: the first sweep of a chain)
    int nreps = 1;
    bool independent_blocks = false, group_launch = false, section_solve = false;
    double pi = 0.0;
    bool use_pi_vec = false, use_pi_mat = false, use_lpr = false;
};

struct SweepPlan {
    enum Path { kIndependent, kGrouped, kLookahead };
    Path path = kLookahead;
    bool dense_big = false, dense_mt = false, dense_mt256 = false, st_helper = false;
    bool gcoop = false, coop = false, pp_want = false, pp_kernel = false;
    int quiet_xcd = 0;              // the sweep's default placement; a launch with a helper or a ping-pong pair forces 1
    int compact_off = 0, dense_big_off = 0, dbg_throttle = 0;
    int64_t solve_blocks = 0;       // Rule T: leading full 256-marker blocks whose section inverses are formed
    uint32_t sched = 0;             // the JWAS_HIP_SCHED_* bits decided per sweep (the launches add QUIET_XCD, GROUP_PINGPONG, CORR_HELPER, DENSE_MT)
};

// The previous sweep changed more than 1.25 % of the markers, or there is none (the first sweep of a chain starts with every marker
// out of or in the model): the sampler chain is the critical path.  Then XCD 0 is kept free of streaming traffic for the sampler; in the
// steady state the sampler has slack and all 8 XCDs stream (+4-5 % bandwidth).  The grouped sweep takes its cooperative apply and its
// ping-pong samplers from the same line (config 3: 25.0 -> 24.3 ms, fixed pi 25.6 -> 25.1 ms per sweep with the cooperative apply).
constexpr double kBusyFraction = 0.0125;
// one block per launch: the update role's column groups share the apply work from a quarter of the markers changed on
constexpr double kCoopFraction = 0.25;
// multi-trait blocks of <= 128 markers: the dense-walk-only sampler once most markers changed last time (the reference's default
// prior: every marker in the model)
constexpr double kDenseMtFraction = 0.6;
// ... of 256-marker blocks: SweepKnobs::dense_mt_fraction (0.1).  The walk costs one step per marker IN the model, so it pays far below
// "most markers change": config 4's chain at 22 000 changes per sweep, 19 ms on the walk against 42 ms through the speculative rounds.
// Blocks of <= 512 markers are only ever grouped for the sampler-bound sweeps: the host keeps those on 512-marker pairs down to 0.9 %
// turnover, and without the ping-pong mode a pair costs 46.9 instead of 40.2 us at 6 300 changes per sweep.
constexpr int kGroupAlwaysBusyBs = 512;

inline bool bs_is_dense_big(int bs) { return bs == 256 || bs == 512; }

inline SweepPlan plan_sweep(const SweepFacts& f, const SweepKnobs& k)
{
    SweepPlan s;
    const bool single_pass = f.nreps == 1 && !f.independent_blocks;
    const bool busy = f.last_events < 0 || f.last_events > kBusyFraction * (double)f.p;
    s.compact_off = k.compact_off;
    s.dense_big_off = k.dense_big_off ? 1 : 0;
    // A uniform prior pi = 0 (single-trait BayesA/B/C: RR-BLUP, BayesA, BayesL): the instantiation whose sampler follows Rule D on every
    // path and takes dense_big_st on full 256- / 512-marker blocks.  Every marker of every block changes.
    s.dense_big = (f.method == JWAS_HIP_BAYESC || f.method == JWAS_HIP_BAYESB) && f.pi == 0.0 && !f.use_pi_vec;
    // full 256-marker blocks of sampler I with one shared covariance (dense_big_mt; a ragged block: launch_dense_mt below)
    s.dense_mt256 = f.bs == 256 && (f.method == JWAS_HIP_MTBAYESC1 || f.method == JWAS_HIP_MTBAYESB1) && !f.use_lpr;
    s.dense_mt = f.multi_trait && !f.sampler2 && (f.bs <= 128 || s.dense_mt256) && single_pass &&
                 (k.dense_mt >= 0 ? k.dense_mt != 0 : f.last_events >= (s.dense_mt256 ? k.dense_mt_fraction : kDenseMtFraction) * (double)f.p);
    // Rule T: multi-trait sampler I with <= 3 traits on uniform 256-marker blocks; every other sweep ignores the flag (4 traits: the
    // sampler has no solve path, and a helper workgroup waiting for sections nobody publishes would spin)
    s.solve_blocks = (f.section_solve && f.t <= 3 && s.dense_mt256 && single_pass && f.uniform && !f.row_mode && !k.dense_big_off) ? f.p / 256 : 0;
    // single-trait dense_big_st blocks hand the next block's lookahead correction to a helper workgroup
    s.st_helper = k.corr_helper != 0 && s.dense_big && single_pass && !f.row_mode && !k.dense_big_off && bs_is_dense_big(f.bs);
    // grouped launches: single-trait single-pass sweeps on uniform blocks; every other sweep ignores the flag
    const bool grouped = f.group_launch && k.groups != 0 && f.gm >= 2 && !f.multi_trait && single_pass && !f.row_mode && f.uniform && !s.dense_big;
    s.path = f.independent_blocks ? SweepPlan::kIndependent : grouped ? SweepPlan::kGrouped : SweepPlan::kLookahead;
    s.sched = (s.dense_big ? JWAS_HIP_SCHED_DENSE_BIG : 0u) | (s.solve_blocks > 0 ? JWAS_HIP_SCHED_SECTION_SOLVE : 0u) |
              (((uint32_t)k.compact_off << JWAS_HIP_SCHED_COMPACT_OFF_SHIFT) & JWAS_HIP_SCHED_COMPACT_OFF_MASK);
    if (s.path == SweepPlan::kIndependent) {
        s.sched |= JWAS_HIP_SCHED_INDEPENDENT;
        return s;
    }
    s.quiet_xcd = k.quiet_xcd >= 0 ? k.quiet_xcd : (busy ? 1 : 0);
    if (s.path == SweepPlan::kGrouped) {
        const bool always = f.bs <= kGroupAlwaysBusyBs;
        // cooperative apply of the merged list: same bits (the chain per row is the list's order either way)
        s.gcoop = f.has_sync_cnt && !f.packed && (k.group_coop >= 0 ? k.group_coop != 0 : (always || busy));
        // ping-pong samplers (2 blocks per launch): JWAS_HIP_PINGPONG=1 also in the steady state, with the quiet XCD forced on
        s.pp_want = f.has_gpp && (k.pingpong >= 0 ? k.pingpong != 0 : (s.quiet_xcd != 0 || always));
        s.pp_kernel = s.pp_want || s.gcoop;
        s.sched |= JWAS_HIP_SCHED_GROUPED | (s.gcoop ? JWAS_HIP_SCHED_GROUP_COOP : 0u) | (s.pp_kernel ? JWAS_HIP_SCHED_GROUP_PP_KERNEL : 0u);
    } else {
        s.coop = f.has_sync_cnt && (k.coop_apply >= 0 ? k.coop_apply != 0 : (s.dense_big || f.last_events > kCoopFraction * (double)f.p));
        s.dbg_throttle = k.debug_throttle;
        s.sched |= s.coop ? JWAS_HIP_SCHED_COOP_APPLY : 0u;
    }
    s.sched |= s.quiet_xcd ? JWAS_HIP_SCHED_QUIET_XCD : 0u;      // (the first launch of either loop runs on the default placement)
    return s;
}

// ---- the three decisions that depend on the block in hand ---------------------------------------------------------------------------
// The dense-walk-only multi-trait instantiation for this launch.  sampling: the launch samples a block (of b markers; every launch but
// a sweep's first).  It serves FULL 256-marker blocks, a ragged last one goes through the general instantiation; Rule T lives in it,
// whatever the last sweep did.
inline bool launch_dense_mt(const SweepPlan& s, int bs, bool sampling, int b, bool rule_t)
{
    if (sampling && rule_t) return true;
    if (s.dense_mt && bs == 256 && sampling) return !s.dense_big_off && b == 256;
    return s.dense_mt;
}

// The sampler hands the next block's correction to the helper workgroup (which lives on the quiet XCD: ids = 0 mod 8 do no streaming).
inline bool launch_uses_helper(const SweepPlan& s, bool rule_t, int bs, int b, int b_next) { return rule_t || (s.st_helper && b == bs && b_next > 0); }

// The group's second block is sampled by its own workgroup: a group of one block has no pair.
inline bool launch_pingpong(const SweepPlan& s, int ns) { return s.pp_want && ns >= 2; }

}  // namespace jw
