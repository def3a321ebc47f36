"""The instantiation table of the fused Lucas-Kanade launchers (mtf_amd/csrc/mtfhip_fused_dispatch.h), checked without a GPU: a
stand-alone host program includes nothing but that header, walks the full cross-product of inputs and prints the key fused_select
chooses; the expected keys below restate the launcher ladders the header replaced, one literal row per case."""
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mtf_amd", "csrc")

SSD, NCC, MI, SCV, RSCV, LSCV, LRSCV = 0, 1, 2, 3, 4, 5, 6      # include/mtfhip.h
LOOP, STEP, PERSIST = 0, 1, 2
REPLAY, FAST_ICLK, FAST_CHAINED, FAST_QSTEP = 0, 1, 2, 3  # RSCV_IT_*

PROGRAM = r"""
#include "mtfhip_fused_dispatch.h"
#include <cstdio>
#include <set>
#include <tuple>
using namespace mtfhip;
typedef std::tuple<int, int, int, int, int, int, int> T;
static T tup(const FusedKey &k) { return T(k.am, k.ssm, k.chained, k.mode, k.mat, k.fast, k.mc); }
static int fails = 0;
/* the visitor hands the key's own fields over as tags, and calls exactly when the unit serves the key */
template <class U> static void visit(const FusedKey &k, bool mine) {
	int calls = 0;
	const bool r = fused_visit<U>(k, [&](auto AM, auto SSM, auto CH, auto MD, auto MAT, auto FAST) {
		++calls;
		if (AM() != k.am || SSM() != k.ssm || CH() != k.chained || MD() != k.mode || MAT() != k.mat || FAST() != k.fast) { ++fails; std::printf("visit: wrong tags\n"); }
	});
	if (r != mine || calls != (mine ? 1 : 0)) { ++fails; std::printf("visit: %d calls, returned %d, expected %d\n", calls, (int)r, (int)mine); }
}
/* fused_reachable against the image of fused_select, key by key; prints the number of instantiations of the unit */
template <class U> static void unit(const char *name, const std::set<T> &image) {
	int n = 0;
	for (int i = 0; i < U::count; ++i) {
		const FusedKey k = U::key(i);
		if (U::index(k) != i) { ++fails; std::printf("unit %s: index(key(%d)) = %d\n", name, i, U::index(k)); }
		const bool r = fused_reachable(U::route, k);
		if (r != (image.count(tup(k)) != 0)) { ++fails; std::printf("unit %s: key %d reachable %d, in the image %d\n", name, i, (int)r, (int)!r); }
		n += r;
	}
	std::printf("unit %s %d\n", name, n);
}
int main() {
	const int ams[] = {MTFHIP_AM_SSD, MTFHIP_AM_NCC, MTFHIP_AM_MI, MTFHIP_AM_SCV, MTFHIP_AM_RSCV, MTFHIP_AM_LSCV, MTFHIP_AM_LRSCV};
	std::set<T> image[3];
	for (int route = 0; route < 3; ++route)
	for (int am : ams) for (int C : {1, 3}) for (int ssm : {MTFHIP_SSM_HOMOGRAPHY, MTFHIP_SSM_AFFINE}) for (int mode = 0; mode < 3; ++mode)
	for (int ch = 0; ch < 2; ++ch) for (int mat = 0; mat < 2; ++mat) for (int fm = 0; fm < 2; ++fm) for (int mapped = 1; mapped >= 0; --mapped) {
		const FusedKey k = fused_select(route, am, C, ssm, mode, ch, mat, fm, mapped);
		std::printf("%d %d %d %d %d %d %d %d %d ->", route, am, C, ssm, mode, ch, mat, fm, mapped);
		if (k.served) std::printf(" %d %d %d %d %d %d %d it%d", k.am, k.ssm, (int)k.chained, k.mode, (int)k.mat, (int)k.fast, (int)k.mc, fused_it_kind(k));
		else std::printf(" none");
		std::printf(" gr%d\n", (int)grid_regen_kernel(am, ssm, ch, mode, mat));
		if (k.served) image[route].insert(tup(k));
		const bool plain = k.served && (k.am == MTFHIP_AM_SSD || k.am == MTFHIP_AM_NCC);
		if (route == FUSED_ROUTE_LOOP) {
			visit<FusedUnit<FUSED_ROUTE_LOOP, false, MTFHIP_AM_SSD, MTFHIP_AM_NCC>>(k, plain && !k.mc);
			visit<FusedUnit<FUSED_ROUTE_LOOP, true, MTFHIP_AM_SSD, MTFHIP_AM_NCC>>(k, plain && k.mc);
			visit<FusedUnit<FUSED_ROUTE_LOOP, false, MTFHIP_AM_RSCV>>(k, k.served && k.am == MTFHIP_AM_RSCV);
			visit<FusedUnit<FUSED_ROUTE_LOOP, false, MTFHIP_AM_LRSCV>>(k, k.served && k.am == MTFHIP_AM_LRSCV);
		} else if (route == FUSED_ROUTE_STEP) visit<FusedUnit<FUSED_ROUTE_STEP, false, MTFHIP_AM_SSD, MTFHIP_AM_NCC>>(k, k.served);
		else visit<FusedUnit<FUSED_ROUTE_PERSIST, false, MTFHIP_AM_SSD, MTFHIP_AM_NCC>>(k, k.served);
	}
	unit<FusedUnit<FUSED_ROUTE_LOOP, false, MTFHIP_AM_SSD, MTFHIP_AM_NCC>>("fused", image[0]);
	unit<FusedUnit<FUSED_ROUTE_LOOP, true, MTFHIP_AM_SSD, MTFHIP_AM_NCC>>("fused_mc", image[0]);
	unit<FusedUnit<FUSED_ROUTE_LOOP, false, MTFHIP_AM_RSCV>>("fused_rscv", image[0]);
	unit<FusedUnit<FUSED_ROUTE_LOOP, false, MTFHIP_AM_LRSCV>>("fused_lrscv", image[0]);
	unit<FusedUnit<FUSED_ROUTE_STEP, false, MTFHIP_AM_SSD, MTFHIP_AM_NCC>>("step", image[1]);
	unit<FusedUnit<FUSED_ROUTE_PERSIST, false, MTFHIP_AM_SSD, MTFHIP_AM_NCC>>("persist", image[2]);
	return fails ? 1 : 0;
}
"""

# (am, channels, mapped) -> the kernel's AM and the multi-channel body, None where nothing is launched.  From launch_fused_ssd: RSCV goes
# to its unit when it has a map and is not launched without; LRSCV with maps goes to its unit, without it falls through to the SSD
# branches; bv.C > 1 goes to the multi-channel unit, where NCC is NCC and everything else SSD; below it NCC is NCC and the rest SSD.
KERNEL_AM = {
    (SSD, 1, 1): (SSD, 0), (SSD, 1, 0): (SSD, 0), (SSD, 3, 1): (SSD, 1), (SSD, 3, 0): (SSD, 1),
    (NCC, 1, 1): (NCC, 0), (NCC, 1, 0): (NCC, 0), (NCC, 3, 1): (NCC, 1), (NCC, 3, 0): (NCC, 1),
    # (MI: mi_enqueue and the lazy MI entry points launch the materialising SSD pass for It / Jt and ignore its sums)
    (MI, 1, 1): (SSD, 0), (MI, 1, 0): (SSD, 0), (MI, 3, 1): (SSD, 1), (MI, 3, 0): (SSD, 1),
    (SCV, 1, 1): (SSD, 0), (SCV, 1, 0): (SSD, 0), (SCV, 3, 1): (SSD, 1), (SCV, 3, 0): (SSD, 1),
    (LSCV, 1, 1): (SSD, 0), (LSCV, 1, 0): (SSD, 0), (LSCV, 3, 1): (SSD, 1), (LSCV, 3, 0): (SSD, 1),
    (RSCV, 1, 1): (RSCV, 0), (RSCV, 1, 0): None, (RSCV, 3, 1): (RSCV, 0), (RSCV, 3, 0): None,
    (LRSCV, 1, 1): (LRSCV, 0), (LRSCV, 1, 0): (SSD, 0), (LRSCV, 3, 1): (LRSCV, 0), (LRSCV, 3, 0): (SSD, 1),
}
# (mode, chained, materialize, fast_math) -> (CHAINED, MODE, MAT, FAST, RSCV_IT_*) on the two-launch route.  From launch_fused_ssd and
# its three siblings: fast_math && !materialize takes the *_fast kernels <MODE, CHAINED> -- mode 2 -> <2, true>, else <mode, chained> --
# and every other launch k_fused_*<CHAINED, MODE, MAT> as given.  The last column is the parent's rscv_it_kind.
LOOP_KEY = {
    (0, 0, 0, 0): (0, 0, 0, 0, REPLAY), (0, 0, 0, 1): (0, 0, 0, 1, FAST_QSTEP), (0, 0, 1, 0): (0, 0, 1, 0, REPLAY), (0, 0, 1, 1): (0, 0, 1, 0, REPLAY),
    (0, 1, 0, 0): (1, 0, 0, 0, REPLAY), (0, 1, 0, 1): (1, 0, 0, 1, FAST_CHAINED), (0, 1, 1, 0): (1, 0, 1, 0, REPLAY), (0, 1, 1, 1): (1, 0, 1, 0, REPLAY),
    (1, 0, 0, 0): (0, 1, 0, 0, REPLAY), (1, 0, 0, 1): (0, 1, 0, 1, FAST_QSTEP), (1, 0, 1, 0): (0, 1, 1, 0, REPLAY), (1, 0, 1, 1): (0, 1, 1, 0, REPLAY),
    (1, 1, 0, 0): (1, 1, 0, 0, REPLAY), (1, 1, 0, 1): (1, 1, 0, 1, FAST_CHAINED), (1, 1, 1, 0): (1, 1, 1, 0, REPLAY), (1, 1, 1, 1): (1, 1, 1, 0, REPLAY),
    (2, 0, 0, 0): (0, 2, 0, 0, REPLAY), (2, 0, 0, 1): (1, 2, 0, 1, FAST_ICLK), (2, 0, 1, 0): (0, 2, 1, 0, REPLAY), (2, 0, 1, 1): (0, 2, 1, 0, REPLAY),
    (2, 1, 0, 0): (1, 2, 0, 0, REPLAY), (2, 1, 0, 1): (1, 2, 0, 1, FAST_ICLK), (2, 1, 1, 0): (1, 2, 1, 0, REPLAY), (2, 1, 1, 1): (1, 2, 1, 0, REPLAY),
}
# the one-launch routes serve single-channel SSD and NCC only (their callers turn the intensity-mapped models and C = 3 away:
# api_track.hip's track_takes_step and persist_fits), with the arguments of LOOP_KEY, and:
# step (track_step_available, launch_track_step): (fast_math && !materialize) -> <MAT = false, FAST = true>, (!fast_math && materialize)
# -> <true, false>, nothing else; persist (launch_track_persist, "fa.materialize must be 0"): FAST = fast_math, never materialising.
STEP_SERVES = {(0, 0): False, (0, 1): True, (1, 0): True, (1, 1): False}      # (materialize, fast_math)
PERSIST_SERVES = {(0, 0): True, (0, 1): True, (1, 0): False, (1, 1): False}
# kernels of fused_lk_body per unit: replay <2 SSM x 2 CHAINED x 3 MODE x 2 MAT> + fast <2 SSM x (2 x 2 + 1)> = 34 per AM; step: 2 AM x
# 2 SSM x (6 materialising replay + 5 fast); persist: 2 AM x 2 SSM x (6 lean replay + 5 fast)
UNIT_KERNELS = {"fused": 68, "fused_mc": 68, "fused_rscv": 34, "fused_lrscv": 34, "step": 44, "persist": 44}


def expected_line(route, am, C, ssm, mode, ch, mat, fm, mapped):
    head = "%d %d %d %d %d %d %d %d %d ->" % (route, am, C, ssm, mode, ch, mat, fm, mapped)
    kam = KERNEL_AM[(am, C, mapped)]
    served = kam is not None
    if route == STEP:
        served = am in (SSD, NCC) and C == 1 and STEP_SERVES[(mat, fm)]
    if route == PERSIST:
        served = am in (SSD, NCC) and C == 1 and PERSIST_SERVES[(mat, fm)]
    # the parent's grid_regen_kernel, SCV and LSCV mapped to SSD as its caller (fused_args) did -- and MI not, so its SSD launches never rebuild
    gr = int(am in (SSD, SCV, LSCV) and ssm == 0 and ch == 1 and mode != 2 and mat == 1)
    if not served:
        return "%s none gr%d" % (head, gr)
    CH, MD, MAT, FAST, it = LOOP_KEY[(mode, ch, mat, fm)]
    return "%s %d %d %d %d %d %d %d it%d gr%d" % (head, kam[0], ssm, CH, MD, MAT, FAST, kam[1], it, gr)


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    d = tmp_path_factory.mktemp("fused_dispatch")
    src, exe = str(d / "t.cpp"), str(d / "t")
    open(src, "w").write(PROGRAM)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, src, "-o", exe],
                   check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:]
    return r.stdout.splitlines()


def test_selected_keys_match_the_ladders_they_replace(table):
    rows = [l for l in table if "->" in l]
    want = [expected_line(*c) for c in itertools.product((LOOP, STEP, PERSIST), (SSD, NCC, MI, SCV, RSCV, LSCV, LRSCV), (1, 3), (0, 1), (0, 1, 2),
                                                         (0, 1), (0, 1), (0, 1), (1, 0))]
    assert len(rows) == len(want) == 3 * 7 * 2 * 2 * 3 * 2 * 2 * 2 * 2
    assert rows == want, [(a, b) for a, b in zip(rows, want) if a != b][:5]


def test_route_predicates(table):
    n_step = n_persist = n_gr = 0
    for l in table:
        if "->" not in l:
            continue
        (route, am, C, ssm, mode, ch, mat, fm, mapped), out = [int(x) for x in l.split(" ->")[0].split()], l.split("-> ")[1].split()
        served = out[0] != "none"
        if route == STEP:
            assert served == (am in (SSD, NCC) and C == 1 and ((fm and not mat) or (not fm and mat))), l
            n_step += served
        if route == PERSIST:
            assert not (served and mat), l
            assert served == (am in (SSD, NCC) and C == 1 and not mat), l
            n_persist += served
        if served:   # FAST is fast_math && !materialize, and a fast ICLK launch is the CHAINED instantiation
            kam, kssm, CH, MD, MAT, FAST, MC = [int(x) for x in out[:7]]
            assert FAST == int(fm and not mat) and MAT == mat and MD == mode and kssm == ssm and CH == int(ch or (FAST and mode == 2)), l
            assert out[7] == "it%d" % (REPLAY if not FAST else FAST_ICLK if mode == 2 else FAST_CHAINED if ch else FAST_QSTEP), l
        gr = out[-1] == "gr1"
        assert gr == (am in (SSD, SCV, LSCV) and ssm == 0 and ch == 1 and mode != 2 and mat == 1), l
        n_gr += gr
    assert n_step and n_persist and n_gr


def test_units_instantiate_what_can_be_launched_and_nothing_else(table):
    """fused_reachable -- the visitor's `if constexpr` -- agrees with the image of fused_select key by key (the program fails otherwise),
    and each unit's count is the number of fused_lk_body kernels it held before, less the <CHAINED = false, MODE = 2, FAST = true> ones of the
    step and persistent units that no launcher reached"""
    got = {l.split()[1]: int(l.split()[2]) for l in table if l.startswith("unit ")}
    assert got == UNIT_KERNELS
