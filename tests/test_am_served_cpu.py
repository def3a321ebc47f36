"""Which appearance model is served where (mtf_amd/csrc/mtfhip_am_served.h), checked without a GPU: a stand-alone host program includes
nothing but that header and prints, for every model and every place, `served` or the refusal's exact text, and every model's traits; the
expected lines are the literal table of tests/helpers/am_served_table.py, typed from the refusal helpers the header replaced.  And over
the text of the sources: those helpers are gone."""
import glob
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mtf_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import am_served_table as T   # noqa: E402

PROGRAM = r"""
#include "mtfhip_am_served.h"
#include <cstdio>
int main() {
	char msg[512];
	for (int am = MTFHIP_AM_SSD; am <= MTFHIP_AM_CCRE; ++am) {
		const AmTraits &t = am_traits(am);
		std::printf("traits %d %s %d %d %d %d %d %d %d %d\n", am, t.name, t.rows, (int)t.intensity_mapped, (int)t.localized, (int)t.reversed,
			(int)t.loop_only, (int)t.hist_driver, t.max_bins, (int)t.bins_default);
		for (int place = 0; place < AM_AT_COUNT; ++place)
			std::printf("%d %d -> %s\n", am, place, am_refused(am, place, "FN", place == AM_AT_ADDITIVE_SM ? "FALK" : nullptr, msg, sizeof(msg)) ? msg : "served");
	}
	/* a buffer too small for the text: cut to cap - 1 characters, terminated, nothing written behind it */
	char small[12] = "...........";
	small[8] = '#';
	const bool r = am_refused(MTFHIP_AM_SCV, AM_AT_GRID, "FN", nullptr, small, 8);
	std::printf("cut %d %s %c\n", (int)r, small, small[8]);
	return 0;
}
"""


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    d = tmp_path_factory.mktemp("am_served")
    src, exe = str(d / "t.cpp"), str(d / "t")
    open(src, "w").write(PROGRAM)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, src, "-o", exe],
                   check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:]
    return r.stdout.splitlines()


def test_the_table_has_every_pair():
    assert set(T.REFUSALS) == {(am, place) for am in T.MODELS for place in T.PLACES}
    assert set(T.TRAITS) == set(T.MODELS) and len(T.PLACES) == 10


def test_served_or_refused_with_the_text_the_helpers_gave(table):
    rows = [l for l in table if " -> " in l]
    want = ["%d %d -> %s" % (am, k, T.REFUSALS[(am, place)] or "served") for am in T.MODELS for k, place in enumerate(T.PLACES)]
    assert len(rows) == len(want) == 100
    assert rows == want, [(a, b) for a, b in zip(rows, want) if a != b][:5]


def test_traits(table):
    rows = [l for l in table if l.startswith("traits ")]
    assert rows == ["traits %d %s %d %d %d %d %d %d %d %d" % ((am,) + T.TRAITS[am]) for am in T.MODELS]


def test_a_short_buffer_cuts_the_text(table):
    assert [l for l in table if l.startswith("cut ")] == ["cut 1 FN: SCV #"]


def test_the_header_needs_no_hip_header():
    text = open(os.path.join(CSRC, "mtfhip_am_served.h")).read()
    assert re.findall(r'#include\s*[<"]([^>"]+)[>"]', text) == ["cstddef", "../../include/mtfhip.h"]


def test_the_refusal_helpers_are_gone():
    """one am_refuse over the table: the five helpers it replaced are named nowhere in csrc, nor their three copies in sm.py"""
    gone = re.compile(r"\b(spss_refuse|ssim_refuse|ccre_refuse|scv_refuse|refuse_intensity_mapped)\b")
    found = {}
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h"))):
        hits = gone.findall(open(path).read())
        if hits:
            found[os.path.basename(path)] = sorted(set(hits))
    assert not found, found
    sm = open(os.path.join(ROOT, "mtf_amd", "sm.py")).read()
    assert not re.findall(r"\b_refuse_(spss|ssim|ccre)\b", sm)
    assert len(re.findall(r"^def _refuse_am\(", sm, re.M)) == 1
