"""The schedule decision of a sweep (csrc/sweep_plan.hpp: plan_sweep, a pure function of SweepFacts and SweepKnobs) on the CPU.

A stand-alone C++ program that includes only that header evaluates the plan for every line of a table and prints the decisions and
the schedule word.  The expected values are written by hand from the documented rules (include/jwas_hip.h): each threshold
from both sides, the first sweep of a chain, each override switch at 0 and 1, everything that switches grouping off, the block-size
clauses, Rule T's conditions.  The chains of tests/test_gpu_schedule_variants.py are rows too -- their per-sweep turnover comes from
that file's docstring -- so this table and the flags observed on the GPU describe the same sweeps."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "jwas.jl_amd", "csrc")

BAYESC, BAYESB, BAYESR, MTC1, MTC2, MEGAC, MTB1 = 0, 1, 2, 3, 4, 5, 6
INDEPENDENT, GROUPED, PP_KERNEL, GROUP_COOP, QUIET, COOP, DENSE_BIG, SOLVE = 1 << 0, 1 << 1, 1 << 2, 1 << 4, 1 << 5, 1 << 6, 1 << 7, 1 << 10
PATH_INDEPENDENT, PATH_GROUPED, PATH_LOOKAHEAD = 0, 1, 2

FACT_KEYS = ["method", "t", "multi_trait", "sampler2", "p", "nblocks", "bs", "uniform", "row_mode", "packed", "gm", "has_gpp", "has_sync_cnt",
             "last_events", "nreps", "independent_blocks", "group_launch", "section_solve", "pi", "use_pi_vec", "use_pi_mat", "use_lpr"]
KNOB_KEYS = ["dense_mt", "dense_big_off", "compact_off", "coop_apply", "dense_mt_fraction", "corr_helper", "groups", "group_coop", "quiet_xcd",
             "pingpong", "debug_throttle"]
OUT_KEYS = ["path", "dense_big", "dense_mt", "dense_mt256", "st_helper", "gcoop", "coop", "pp_want", "pp_kernel", "quiet_xcd", "compact_off",
            "dense_big_off", "dbg_throttle", "solve_blocks", "sched", "dmt_full", "dmt_ragged", "dmt_first", "dmt_rule_t", "helper_full",
            "helper_ragged", "helper_last", "helper_rule_t", "pp1", "pp2"]

PROGRAM = r"""
#include "sweep_plan.hpp"
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
using namespace jw;
static void print_knobs(const SweepKnobs& k)
{
    std::printf("dense_mt=%d dense_big_off=%d compact_off=%d coop_apply=%d debug_phases=%d dense_mt_fraction=%g corr_helper=%d groups=%d "
                "group_coop=%d quiet_xcd=%d pingpong=%d debug_throttle=%d\n", k.dense_mt, (int)k.dense_big_off, k.compact_off, k.coop_apply,
                (int)k.debug_phases, k.dense_mt_fraction, k.corr_helper, k.groups, k.group_coop, k.quiet_xcd, k.pingpong, k.debug_throttle);
}
int main(int argc, char** argv)
{
    if (argc > 1) {          // the switches: from the environment, then again after every one of them changed
        print_knobs(sweep_knobs());
        for (const char* name : {"DENSE_MT", "DENSE_BIG_OFF", "COMPACT_OFF", "COOP_APPLY", "DEBUG_PHASES", "DENSE_MT_FRACTION", "CORR_HELPER",
                                 "GROUPS", "GROUP_COOP", "QUIET_XCD", "PINGPONG", "DEBUG_THROTTLE"})
            setenv((std::string("JWAS_HIP_") + name).c_str(), "3", 1);
        print_knobs(sweep_knobs());
        return 0;
    }
    std::string line;
    while (std::getline(std::cin, line)) {
        SweepFacts f;
        SweepKnobs k;
        std::istringstream in(line);
        std::string tok;
        while (in >> tok) {
            const size_t eq = tok.find('=');
            const std::string key = tok.substr(0, eq);
            const double v = std::atof(tok.c_str() + eq + 1);
#define FACT(name) else if (key == #name) f.name = (decltype(f.name))v;
#define KNOB(name) else if (key == "knob." #name) k.name = (decltype(k.name))v;
            if (key.empty()) return 2;
            FACT(method) FACT(t) FACT(multi_trait) FACT(sampler2) FACT(p) FACT(nblocks) FACT(bs) FACT(uniform) FACT(row_mode) FACT(packed)
            FACT(gm) FACT(has_gpp) FACT(has_sync_cnt) FACT(last_events) FACT(nreps) FACT(independent_blocks) FACT(group_launch)
            FACT(section_solve) FACT(pi) FACT(use_pi_vec) FACT(use_pi_mat) FACT(use_lpr)
            KNOB(dense_mt) KNOB(dense_big_off) KNOB(compact_off) KNOB(coop_apply) KNOB(dense_mt_fraction) KNOB(corr_helper) KNOB(groups)
            KNOB(group_coop) KNOB(quiet_xcd) KNOB(pingpong) KNOB(debug_throttle)
            else { std::fprintf(stderr, "unknown key %s\n", key.c_str()); return 2; }
        }
        const SweepPlan s = plan_sweep(f, k);
        std::printf("path=%d dense_big=%d dense_mt=%d dense_mt256=%d st_helper=%d gcoop=%d coop=%d pp_want=%d pp_kernel=%d quiet_xcd=%d "
                    "compact_off=%d dense_big_off=%d dbg_throttle=%d solve_blocks=%lld sched=%u ",
                    s.path == SweepPlan::kIndependent ? 0 : s.path == SweepPlan::kGrouped ? 1 : 2, (int)s.dense_big, (int)s.dense_mt,
                    (int)s.dense_mt256, (int)s.st_helper, (int)s.gcoop, (int)s.coop, (int)s.pp_want, (int)s.pp_kernel, s.quiet_xcd,
                    s.compact_off, s.dense_big_off, s.dbg_throttle, (long long)s.solve_blocks, s.sched);
        // the per-launch decisions: a full block, a ragged one, the first launch (no sampler), a Rule T block; a single block, a pair
        std::printf("dmt_full=%d dmt_ragged=%d dmt_first=%d dmt_rule_t=%d helper_full=%d helper_ragged=%d helper_last=%d helper_rule_t=%d pp1=%d pp2=%d\n",
                    (int)launch_dense_mt(s, f.bs, true, f.bs, false), (int)launch_dense_mt(s, f.bs, true, f.bs - 7, false),
                    (int)launch_dense_mt(s, f.bs, false, 0, false), (int)launch_dense_mt(s, f.bs, true, f.bs, true),
                    (int)launch_uses_helper(s, false, f.bs, f.bs, f.bs), (int)launch_uses_helper(s, false, f.bs, f.bs - 7, f.bs),
                    (int)launch_uses_helper(s, false, f.bs, f.bs, 0), (int)launch_uses_helper(s, true, f.bs, f.bs - 7, 0),
                    (int)launch_pingpong(s, 1), (int)launch_pingpong(s, 2));
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("sweep_plan")
    (d / "plan.cpp").write_text(PROGRAM)
    exe = str(d / "plan")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, str(d / "plan.cpp"), "-o", exe])
    return exe


def _kv(text):
    return {k: float(v) for k, v in (tok.split("=") for tok in text.split())}


def _plan(program, rows):
    lines = []
    for facts, knobs, _ in rows:
        assert set(facts) <= set(FACT_KEYS) and set(knobs) <= set(KNOB_KEYS)
        lines.append(" ".join([f"{k}={float(v)!r}" for k, v in facts.items()] + [f"knob.{k}={float(v)!r}" for k, v in knobs.items()]))
    out = subprocess.run([program], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(rows)
    return [_kv(line) for line in out]


def _check(program, rows):
    for (facts, knobs, want), got in zip(rows, _plan(program, rows)):
        assert sorted(got) == sorted(OUT_KEYS)
        for k, v in want.items():
            assert got[k] == v, (facts, knobs, k, got[k], v)


# ---- the facts of the chains of tests/_schedule_worker.py ------------------------------------------------------------------------------
def grouped(m, last, p=None, bs=1024, **kw):
    p = p or 1024 * (2 * m + 1) + 24
    return dict(dict(method=BAYESC, p=p, bs=bs, nblocks=-(-p // bs), gm=m, has_gpp=1, has_sync_cnt=1, group_launch=1, pi=0.9, last_events=last), **kw)


def lookahead(last, p=2600, bs=512, **kw):
    return dict(dict(method=BAYESC, p=p, bs=bs, nblocks=-(-p // bs), has_sync_cnt=1, pi=0.4, last_events=last), **kw)


def mt(bs, last, p, t=2, method=MTC1, **kw):
    return dict(dict(method=method, t=t, multi_trait=1, p=p, bs=bs, nblocks=-(-p // bs), has_sync_cnt=1, last_events=last), **kw)


def test_thresholds_from_both_sides(program):
    p = 5144                                                   # 1.25 % of p = 64.3
    busy = dict(path=PATH_GROUPED, gcoop=1, pp_want=1, pp_kernel=1, quiet_xcd=1, sched=GROUPED | GROUP_COOP | PP_KERNEL | QUIET, pp1=0, pp2=1)
    steady = dict(path=PATH_GROUPED, gcoop=0, pp_want=0, pp_kernel=0, quiet_xcd=0, sched=GROUPED, pp1=0, pp2=0)
    p2 = 2600                                                  # 25 % = 650, 1.25 % = 32.5
    rows = [
        (grouped(2, 65), {}, busy), (grouped(2, 64), {}, steady),
        (grouped(2, -1), {}, busy),                            # the first sweep of a chain
        (lookahead(651), {}, dict(path=PATH_LOOKAHEAD, coop=1, quiet_xcd=1, sched=COOP | QUIET)),
        (lookahead(650), {}, dict(coop=0, quiet_xcd=1, sched=QUIET)),
        (lookahead(33), {}, dict(coop=0, quiet_xcd=1, sched=QUIET)), (lookahead(32), {}, dict(coop=0, quiet_xcd=0, sched=0)),
        (lookahead(-1), {}, dict(coop=0, quiet_xcd=1, sched=QUIET)),          # no count yet: the cooperative apply off, the quiet XCD on
        # the dense walk: 60 % of p on blocks of <= 128 markers (p 401: 240.6), 10 % on 256-marker blocks (p 785: 78.5), >= either
        (mt(128, 241, 401), {}, dict(dense_mt=1, dense_mt256=0, dmt_full=1, dmt_ragged=1, dmt_first=1)),
        (mt(128, 240, 401), {}, dict(dense_mt=0, dmt_full=0, dmt_first=0)),
        (mt(256, 79, 785), {}, dict(dense_mt=1, dense_mt256=1, dmt_full=1, dmt_ragged=0, dmt_first=1)),
        (mt(256, 78, 785), {}, dict(dense_mt=0, dense_mt256=1, dmt_full=0)),
        (mt(256, 79, 785), dict(dense_mt_fraction=0.2), dict(dense_mt=0)),       # the fraction moved: 20 % = 157
        (mt(256, 157, 785), dict(dense_mt_fraction=0.2), dict(dense_mt=1)),
        (mt(256, 156, 785), dict(dense_mt_fraction=0.2), dict(dense_mt=0)),
        (mt(128, 200, 401), dict(dense_mt_fraction=0.2), dict(dense_mt=0)),      # (blocks of 128 markers keep their 60 %)
        (mt(128, -1, 401), {}, dict(dense_mt=0, quiet_xcd=1)),
        (mt(512, 785, 785), {}, dict(dense_mt=0, dense_mt256=0)),                 # neither <= 128 nor 256
        (mt(128, 401, 401, method=MTC2, sampler2=1), {}, dict(dense_mt=0)),
        (mt(256, 785, 785, use_lpr=1), {}, dict(dense_mt=0, dense_mt256=0)),
        (mt(128, 401, 401, nreps=2), {}, dict(dense_mt=0)),
    ]
    _check(program, rows)


def test_the_chains_of_the_schedule_tests(program):
    """Per-sweep turnover in % of p from the docstring of tests/test_gpu_schedule_variants.py; sweep s follows sweep s - 1."""
    def rows_of(pct, make, p, want):
        last = [-1.0] + [x * p / 100.0 for x in pct[:-1]]
        return [(make(v), {}, want(s)) for s, v in enumerate(last, 1)]

    g2 = [8.26, 8.32, 0.23, 0.23, 0.25, 0.19, 5.73, 10.81, 6.12, 0.27, 0.17, 0.17]
    g4 = [8.63, 8.71, 0.32, 0.24, 0.21, 0.18, 6.56, 12.65, 7.15, 0.22, 0.21, 0.19]
    high = {1, 2, 3, 8, 9, 10}                                 # "sweeps 1-3 and 8-10 run k_group_step<.., true>"
    gw = lambda s: dict(path=PATH_GROUPED, sched=(GROUPED | GROUP_COOP | PP_KERNEL | QUIET) if s in high else GROUPED)
    la = [52.1, 73.9, 54.2, 16.2, 8.27, 0.50, 0.42, 0.42, 0.42, 46.9, 71.1, 72.8]
    lw = lambda s: dict(path=PATH_LOOKAHEAD, coop=int(s in (2, 3, 4, 11, 12)), quiet_xcd=int(s not in (7, 8, 9, 10)))
    m128 = [100, 100, 100, 100, 25.9, 4.49, 2.74, 2.00, 44.6, 65.8, 77.6, 86.3]
    m256 = [100, 100, 100, 100, 28.0, 3.69, 1.53, 1.02, 44.7, 68.2, 80.4, 87.8]
    rows = (rows_of(g2, lambda v: grouped(2, v), 5144, gw) + rows_of(g4, lambda v: grouped(4, v), 9240, gw) +
            rows_of(g2, lambda v: grouped(2, v, method=BAYESR), 5144, gw) +
            # packed storage: no cooperative apply of the merged list, the ping-pong kernel all the same
            rows_of(g2, lambda v: grouped(2, v, packed=1), 5144,
                    lambda s: dict(gcoop=0, sched=(GROUPED | PP_KERNEL | QUIET) if s in high else GROUPED)) +
            rows_of(la, lookahead, 2600, lw) +
            rows_of(m128, lambda v: mt(128, v, 401), 401, lambda s: dict(dense_mt=int(s in (2, 3, 4, 5, 11, 12)))) +
            rows_of(m256, lambda v: mt(256, v, 785), 785, lambda s: dict(dense_mt=int(s in (2, 3, 4, 5, 6, 10, 11, 12)))) +
            # pi = 0: dense_big, the cooperative apply and the helper workgroup in every sweep, the first included
            [(lookahead(v, p=808, bs=256, pi=0.0), {}, dict(dense_big=1, st_helper=1, coop=1, helper_full=1, helper_ragged=0, helper_last=0,
                                                            sched=DENSE_BIG | COOP | QUIET)) for v in (-1, 808)])
    _check(program, rows)


def test_override_switches(program):
    low, high = grouped(2, 10), grouped(2, 1000)
    rows = [
        (low, dict(group_coop=1), dict(gcoop=1, pp_want=0, pp_kernel=1, quiet_xcd=0, sched=GROUPED | GROUP_COOP | PP_KERNEL)),
        (high, dict(group_coop=0), dict(gcoop=0, pp_want=1, pp_kernel=1, sched=GROUPED | PP_KERNEL | QUIET)),
        (low, dict(pingpong=1), dict(pp_want=1, gcoop=0, pp_kernel=1, quiet_xcd=0, sched=GROUPED | PP_KERNEL, pp2=1, pp1=0)),
        (high, dict(pingpong=0), dict(pp_want=0, gcoop=1, pp_kernel=1, sched=GROUPED | GROUP_COOP | PP_KERNEL | QUIET, pp2=0)),
        (low, dict(quiet_xcd=1), dict(quiet_xcd=1, pp_want=1, gcoop=0, sched=GROUPED | PP_KERNEL | QUIET)),
        (high, dict(quiet_xcd=0), dict(quiet_xcd=0, pp_want=0, gcoop=1, sched=GROUPED | GROUP_COOP | PP_KERNEL)),
        (high, dict(groups=0), dict(path=PATH_LOOKAHEAD, gcoop=0, pp_want=0, sched=QUIET)),
        (lookahead(10), dict(coop_apply=1), dict(coop=1, sched=COOP)), (lookahead(2000), dict(coop_apply=0), dict(coop=0, sched=QUIET)),
        (lookahead(10, has_sync_cnt=0), dict(coop_apply=1), dict(coop=0)),
        (lookahead(10), dict(quiet_xcd=1), dict(quiet_xcd=1)), (lookahead(2000), dict(quiet_xcd=0), dict(quiet_xcd=0, sched=COOP)),
        (mt(128, 0, 401), dict(dense_mt=1), dict(dense_mt=1)), (mt(128, 401, 401), dict(dense_mt=0), dict(dense_mt=0)),
        (mt(128, 0, 401, independent_blocks=1), dict(dense_mt=1), dict(dense_mt=0, path=PATH_INDEPENDENT)),
        (lookahead(10), dict(compact_off=1), dict(compact_off=1, sched=1 << 11)), (lookahead(10), dict(compact_off=3), dict(compact_off=3, sched=3 << 11)),
        (lookahead(10), dict(compact_off=0), dict(compact_off=0, sched=0)),
        (lookahead(10), dict(debug_throttle=4), dict(dbg_throttle=4)), (low, dict(debug_throttle=4), dict(dbg_throttle=0)),
        # the helper workgroup of the dense single-trait sweeps, and the switch that sends the same chain through the general path
        (lookahead(808, p=808, bs=256, pi=0.0), dict(corr_helper=0), dict(dense_big=1, st_helper=0, helper_full=0, sched=DENSE_BIG | COOP | QUIET)),
        (lookahead(808, p=808, bs=256, pi=0.0), dict(dense_big_off=1), dict(dense_big=1, st_helper=0, dense_big_off=1, sched=DENSE_BIG | COOP | QUIET)),
        (lookahead(808, p=808, bs=128, pi=0.0), {}, dict(dense_big=1, st_helper=0)),
        (lookahead(808, p=808, bs=256, pi=0.0, row_mode=1), {}, dict(dense_big=1, st_helper=0)),
        (lookahead(808, p=808, bs=256, pi=0.0, use_pi_vec=1), {}, dict(dense_big=0, st_helper=0)),
        (lookahead(808, p=808, bs=256, pi=0.0, method=BAYESR), {}, dict(dense_big=0)),
        (lookahead(808, p=808, bs=256, pi=0.0, method=BAYESB), {}, dict(dense_big=1, st_helper=1)),
        (mt(256, 785, 785), dict(dense_big_off=1), dict(dense_mt=1, dmt_full=0, dmt_ragged=0, dmt_first=1)),
    ]
    _check(program, rows)


def test_what_switches_grouping_off(program):
    on = dict(path=PATH_GROUPED)
    off = dict(path=PATH_LOOKAHEAD, gcoop=0, pp_want=0, pp_kernel=0)
    rows = [
        (grouped(2, 1000), {}, on), (grouped(4, 1000), {}, on),
        (grouped(2, 1000, group_launch=0), {}, off), (grouped(1, 1000), {}, off), (grouped(0, 1000), {}, off),
        (grouped(2, 1000, method=MTC1, t=2, multi_trait=1), {}, off), (grouped(2, 1000, method=MEGAC, t=2, multi_trait=1), {}, off),
        (grouped(2, 1000, nreps=2), {}, off), (grouped(2, 1000, row_mode=1), {}, off), (grouped(2, 1000, uniform=0), {}, off),
        (grouped(2, 1000, pi=0.0), {}, dict(off, dense_big=1)),
        (grouped(2, 1000, pi=0.0, use_pi_vec=1), {}, on),      # (per-marker priors: not dense_big)
        (grouped(2, 1000, independent_blocks=1), {}, dict(path=PATH_INDEPENDENT, sched=INDEPENDENT, quiet_xcd=0, coop=0, gcoop=0)),
    ]
    _check(program, rows)


def test_small_blocks_are_grouped_for_the_sampler_bound_sweeps(program):
    """bs <= 512: the cooperative apply and the ping-pong samplers whatever the last sweep's count was."""
    p = 512 * 5 + 24
    rows = [
        (grouped(2, 0, p=p, bs=512), {}, dict(gcoop=1, pp_want=1, pp_kernel=1, quiet_xcd=0, sched=GROUPED | GROUP_COOP | PP_KERNEL)),
        (grouped(2, 0, p=p, bs=513), {}, dict(gcoop=0, pp_want=0, pp_kernel=0, sched=GROUPED)),
        (grouped(2, 0, p=p, bs=512, has_gpp=0), {}, dict(gcoop=1, pp_want=0, pp_kernel=1)),
        (grouped(2, 0, p=p, bs=512, has_sync_cnt=0), {}, dict(gcoop=0, pp_want=1, pp_kernel=1)),
        (grouped(2, 0, p=p, bs=512, packed=1), {}, dict(gcoop=0, pp_want=1)),
        (grouped(2, 0, p=p, bs=512), dict(group_coop=0, pingpong=0), dict(gcoop=0, pp_want=0, pp_kernel=0, sched=GROUPED)),
    ]
    _check(program, rows)


def test_rule_t(program):
    full = dict(section_solve=1)
    rows = [
        (mt(256, 0, 785, t=2, **full), {}, dict(solve_blocks=3, sched=SOLVE, dmt_rule_t=1, helper_rule_t=1, dense_mt=0, dmt_full=0)),
        (mt(256, 0, 785, t=3, **full), {}, dict(solve_blocks=3)), (mt(256, 0, 785, t=3, method=MTB1, **full), {}, dict(solve_blocks=3)),
        (mt(256, 0, 1024, t=2, **full), {}, dict(solve_blocks=4)),
        (mt(256, 0, 785, t=4, **full), {}, dict(solve_blocks=0, sched=0)),
        (mt(256, 0, 785, uniform=0, **full), {}, dict(solve_blocks=0)),
        (mt(256, 0, 785, **full), dict(dense_big_off=1), dict(solve_blocks=0)),
        (mt(256, 0, 785), {}, dict(solve_blocks=0)), (mt(128, 0, 785, **full), {}, dict(solve_blocks=0)),
        (mt(256, 0, 785, method=MTC2, sampler2=1, **full), {}, dict(solve_blocks=0)), (mt(256, 0, 785, use_lpr=1, **full), {}, dict(solve_blocks=0)),
        (mt(256, 0, 785, nreps=2, **full), {}, dict(solve_blocks=0)), (mt(256, 0, 785, row_mode=1, **full), {}, dict(solve_blocks=0)),
        (mt(256, 0, 785, independent_blocks=1, **full), {}, dict(solve_blocks=0, sched=INDEPENDENT)),
    ]
    _check(program, rows)


def test_switches_read_per_process_and_per_sweep(program):
    """sweep_knobs(): the defaults, the environment, and which switches a second read in the same process sees changed."""
    names = ["DENSE_MT", "DENSE_BIG_OFF", "COMPACT_OFF", "COOP_APPLY", "DEBUG_PHASES", "DENSE_MT_FRACTION", "CORR_HELPER", "GROUPS", "GROUP_COOP",
             "QUIET_XCD", "PINGPONG", "DEBUG_THROTTLE"]
    env = {k: v for k, v in os.environ.items() if not k.startswith("JWAS_HIP_")}
    run = lambda e: [_kv(line) for line in subprocess.run([program, "knobs"], env=e, capture_output=True, text=True, check=True).stdout.splitlines()]
    defaults = dict(dense_mt=-1, dense_big_off=0, compact_off=0, coop_apply=-1, debug_phases=0, dense_mt_fraction=0.1, corr_helper=1, groups=1,
                    group_coop=-1, quiet_xcd=-1, pingpong=-1, debug_throttle=0)
    per_sweep = dict(dense_mt=3, dense_big_off=1, compact_off=3, coop_apply=3, debug_phases=1)
    first, second = run(env)
    assert first == defaults
    assert second == dict(defaults, **per_sweep)                # the program set every switch to 3 between the two reads
    first, second = run(dict(env, **{"JWAS_HIP_" + n: "0" for n in names}))
    # (JWAS_HIP_DEBUG_THROTTLE: development builds only; a switch that is merely SET counts as on)
    assert first == dict(dense_mt=0, dense_big_off=1, compact_off=0, coop_apply=0, debug_phases=1, dense_mt_fraction=0.0, corr_helper=0, groups=0,
                         group_coop=0, quiet_xcd=0, pingpong=0, debug_throttle=0)
    assert second == dict(first, **per_sweep)
