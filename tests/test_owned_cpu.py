"""The owner types of the handles (mtf_amd/csrc/mtfhip_owned.h), checked without a GPU: a stand-alone host program includes nothing but
that header, gives it a counting memory policy that can fail the k-th allocation and throw from its release, and runs under the address
and undefined-behaviour sanitizers as a process of its own.  And the rule the types exist for, over the text of csrc: the runtime's
allocation, event and stream calls appear where the policies are defined and nowhere else."""
import glob
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mtf_amd", "csrc")

PROGRAM = r"""
#include "mtfhip_owned.h"
#include <cstdio>
#include <cstdlib>
#include <set>
#include <stdexcept>
using namespace mtfhip;

static int fails = 0;
#define CHECK(x) do { if (!(x)) { ++fails; std::printf("line %d: %s\n", __LINE__, #x); } } while (0)

/* counts live blocks, fails the fail_at-th allocation from now (1 = the next one), can throw from release; a block released twice or
 * never is also the sanitizer's finding (malloc / free underneath) */
struct Fake {
	static std::set<void *> live;
	static int allocs, releases, fail_at;
	static bool throwing;
	static int alloc(void **p, size_t bytes) {
		if (fail_at > 0 && --fail_at == 0) return 2;
		*p = std::malloc(bytes ? bytes : 1);
		live.insert(*p); ++allocs;
		return 0;
	}
	static void release(void *p) {
		if (live.erase(p) != 1) { ++fails; std::printf("release of a block that is not live\n"); return; }
		std::free(p); ++releases;
		if (throwing) throw std::runtime_error("the runtime is going away");
	}
};
std::set<void *> Fake::live;
int Fake::allocs = 0, Fake::releases = 0, Fake::fail_at = 0;
bool Fake::throwing = false;
typedef Owned<double, Fake> Buf;

struct FakeApi {
	typedef int handle;
	static int next, live_handles;
	static bool throwing;
	static int create(int *h, unsigned flags = 0) { if (flags == 99) return 3; *h = ++next; ++live_handles; return 0; }
	static void destroy(int) { --live_handles; if (throwing) throw std::runtime_error("the runtime is going away"); }
};
int FakeApi::next = 0, FakeApi::live_handles = 0;
bool FakeApi::throwing = false;
typedef OwnedHandle<FakeApi> Handle;

static double *as_pointer(double *p) { return p; }

int main() {
	{
		Buf a;
		CHECK(!a && a.get() == nullptr && a.capacity() == 0);
		CHECK(a.reserve(0) == 0 && Fake::allocs == 0);                      /* nothing asked, nothing done */
		CHECK(a.reserve(10) == 0 && a && a.capacity() == 10 && Fake::allocs == 1 && Fake::live.size() == 1);
		double *p = a;
		a[9] = 1.0; *a = 2.0;                                               /* reads as a pointer: subscript, dereference, */
		CHECK(as_pointer(a) == p && a + 3 == p + 3 && a == p);              /* argument, arithmetic, comparison */
		CHECK(a.reserve(10) == 0 && a.reserve(4) == 0 && a.get() == p && a.capacity() == 10 && Fake::allocs == 1 && Fake::releases == 0);
		CHECK(a.reserve(11) == 0 && a.capacity() == 11 && Fake::allocs == 2 && Fake::releases == 1 && Fake::live.size() == 1);
		/* a failed grow: the policy's error, {nullptr, 0}, the old block released exactly once */
		Fake::fail_at = 1;
		CHECK(a.reserve(100) == 2 && !a && a.capacity() == 0 && Fake::releases == 2 && Fake::live.empty());
		/* ... and a smaller request then allocates instead of trusting the old capacity */
		CHECK(a.reserve(5) == 0 && a && a.capacity() == 5 && Fake::allocs == 3 && Fake::live.size() == 1);
		/* move and swap carry pointer and capacity together */
		Buf b;
		CHECK(b.reserve(7) == 0);
		double *pa = a, *pb = b;
		a.swap(b);
		CHECK(a.get() == pb && a.capacity() == 7 && b.get() == pa && b.capacity() == 5);
		swap(a, b);
		CHECK(a.get() == pa && a.capacity() == 5 && b.get() == pb && b.capacity() == 7);
		Buf c(std::move(a));
		CHECK(!a && a.capacity() == 0 && c.get() == pa && c.capacity() == 5 && Fake::live.size() == 2);
		b = std::move(c);                                                   /* b's own block goes, c's arrives */
		CHECK(!c && c.capacity() == 0 && b.get() == pa && b.capacity() == 5 && Fake::live.size() == 1 && Fake::live.count(pa) == 1);
		b = std::move(b);                                                   /* (self-assignment keeps it) */
		CHECK(b.get() == pa && b.capacity() == 5 && Fake::live.size() == 1);
		b.reset(); b.reset();
		CHECK(!b && b.capacity() == 0 && Fake::live.empty());
		/* a release that throws is swallowed by reset() and by the destructor */
		CHECK(a.reserve(3) == 0 && c.reserve(3) == 0);
		Fake::throwing = true;
		a.reset();
		CHECK(!a && a.capacity() == 0 && Fake::live.size() == 1);
	}                                                                       /* (c's destructor, still throwing) */
	Fake::throwing = false;
	CHECK(Fake::live.empty() && Fake::allocs == Fake::releases);
	{
		Handle none, own, lent;
		CHECK(!none && !none.owned());
		CHECK(own.create() == 0 && own && own.owned() && FakeApi::live_handles == 1);
		CHECK(none.create(99u) == 3 && !none && !none.owned() && FakeApi::live_handles == 1);   /* a failed create leaves nothing */
		lent.borrow(1234);
		CHECK(lent.get() == 1234 && !lent.owned());
		const int h = own;
		Handle moved(std::move(own));
		CHECK(!own && !own.owned() && moved.get() == h && moved.owned() && FakeApi::live_handles == 1);
		lent = std::move(moved);                                            /* the borrowed handle is dropped, not destroyed */
		CHECK(lent.get() == h && lent.owned() && FakeApi::live_handles == 1);
		lent.borrow(77);                                                    /* ... and the owned one is destroyed when it is replaced */
		CHECK(FakeApi::live_handles == 0 && lent.get() == 77);
		lent.reset();
		CHECK(FakeApi::live_handles == 0 && !lent);
		CHECK(own.create(1u) == 0);
		FakeApi::throwing = true;
	}                                                                       /* (own's destructor, throwing) */
	FakeApi::throwing = false;
	CHECK(FakeApi::live_handles == 0);
	std::printf("live %zu allocs %d releases %d handles %d\n", Fake::live.size(), Fake::allocs, Fake::releases, FakeApi::live_handles);
	return fails ? 1 : 0;
}
"""


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    d = tmp_path_factory.mktemp("owned")
    src, exe = str(d / "t.cpp"), str(d / "t")
    open(src, "w").write(PROGRAM)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-self-move", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, src, "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:]
    return r.stdout.splitlines()


def test_owner_types_under_a_counting_policy(report):
    """every CHECK of the program held (it exits 1 otherwise), nothing is live at exit and every block was released exactly once"""
    assert report == ["live 0 allocs 6 releases 6 handles 0"]


def test_the_owner_header_needs_no_hip_header():
    text = open(os.path.join(CSRC, "mtfhip_owned.h")).read()
    assert re.findall(r'#include\s*[<"]([^>"]+)[>"]', text) == ["cstddef", "utility"]


# the functions of the runtime that obtain or release device memory, pinned memory, events and streams: the bare names, so that an
# address taken, a macro around one, a comment or a message that names one counts as well
CALLS = re.compile(r"\b(hipMalloc\w*|hipExtMalloc\w*|hipFree\w*|hipHostMalloc|hipHostAlloc|hipHostFree|hipEventCreate\w*|hipEventDestroy|"
                   r"hipStreamCreate\w*|hipStreamDestroy)\b")
POLICIES = ("DeviceMem", "PinnedMem", "FineGrainedMem", "EventApi", "StreamApi")


def test_allocation_calls_live_in_the_policies_only():
    """mtf_amd/csrc names those functions inside the bodies of the policy structs of mtfhip_internal.h -- what the owners are built on --
    and nowhere else: a new buffer, event or stream is a member of an owner type, not one more line of a free list"""
    found = {}
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h"))):
        text = open(path).read()
        name = os.path.basename(path)
        spans = []
        if name == "mtfhip_internal.h":
            for p in POLICIES:
                m = re.search(r"\bstruct %s \{.*?\n\};" % p, text, re.S)
                assert m, "policy %s is not defined in mtfhip_internal.h" % p
                assert CALLS.search(m.group(0)), "policy %s makes no runtime call" % p
                spans.append(m.span())
        for m in CALLS.finditer(text):
            if not any(a <= m.start() < b for a, b in spans):
                found.setdefault(name, []).append("%s (line %d)" % (m.group(1), text.count("\n", 0, m.start()) + 1))
    assert not found, found
