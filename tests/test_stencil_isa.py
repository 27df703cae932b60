"""The stencil's LDS input ring waits for its rows by count (CPU: hipcc cross-compiles gfx950 here).

The stencil's input rows reach a per-wave LDS ring of QD = LLFE_ST_LDSQ rows by 12-byte
direct-to-LDS loads issued QD - 1 row steps ahead.  The compiler does not track
those loads: the kernel itself waits for a row with a hand-placed ``s_waitcnt`` before it reads
it.  Vector-memory operations complete in order, so a counted wait ``vmcnt(N)``, N > 0, proves a
row landed only if N younger operations were issued after that row's load -- which holds in the
steady state, where the step has just issued its own load, and not in a segment's last QD - 1
steps, which issue none.  There the wait must drain, ``vmcnt(0)``.  A read placed by a count that
is not there passes every parity run while the load happens to land first, so the ISA is the
guard, not a clean run.

For all six kernels the library ships (k_stencil_stream and k_stencil_images, each as <1,1>,
<1,0> and <0,1>), compiled with the flags build() uses (_build.compile_flags), this test splits
the function into basic blocks (labels, branches, fall-through) and walks backwards from every
ring read -- any LDS read: the interior wave's ``ds_read_b96`` of the lane's slot and the border
wave's byte gathers -- along every path, up to the previous ring read or the function's entry:

  * the first ``s_waitcnt`` with a vmcnt met on a path is ``vmcnt(0)``, or
  * it is ``vmcnt(N)``, 0 < N <= QD - 2, and every path into that wait issued a direct-to-LDS
    load after the previous ring read, i.e. this step's load (``global_load_lds_dwordx3`` for
    interior waves, ``buffer_load_dwordx3 ... lds`` for border waves);
  * no path issues a direct-to-LDS load and then reads the ring with no wait at all;
  * every read that opens a step's ring reads (the interior read; the first byte of a border
    gather) has, on some path in front of it, the kernel's own drain -- a ``vmcnt(0)`` that can
    be reached from the previous ring read, or the entry, without any vector-memory load in
    between -- and, on another, a counted wait behind the step's load.

The last rule is what holds the tail's wait in place.  The walk cannot know ``vec``: a path with
neither load nor wait must be let through, because waves of unaligned images (``vec`` false)
take it in the tail -- their rows were written with ordinary LDS stores, which the compiler
tracks.  With the tail's drain deleted, a ``vec`` wave takes the same path, and the first three
rules alone would not see it.  Nor may any ``vmcnt(0)`` do: the compiler puts one of its own
behind the byte path's ordinary loads in every step, and that one waits for those loads, not for
the ring.  The drain that counts is the one no load of the step precedes.

The walk follows every edge of the control-flow graph whether or not its condition can hold
together with the others on the path, so the kernel keeps each counted wait in the arm that
issues the load.  The older assertions stay: at least 12 loads of each direct-to-LDS form and one
ring read per unrolled row step.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "low_level_feature_extraction_amd", "csrc", "stencil_stream.hip")

KERNELS = [f"{k}ILb{c}ELb{s}E" for k in ("k_stencil_stream", "k_stencil_images") for c, s in ((1, 1), (1, 0), (0, 1))]

_BRANCH = re.compile(r"^s_(c?branch)\w*\s+(\.L\S+)")
_LABEL = re.compile(r"^(\.L\w+):")
_VMWAIT = re.compile(r"^s_waitcnt\b.*\bvmcnt\((\d+)\)")
_RING_READ = re.compile(r"^ds_read\w*\b")
_INTERIOR_READ = re.compile(r"^(ds_read_b96|ds_read2_b32)\b")
_LDS_LOAD = re.compile(r"^(global_load_lds_\w+\b|buffer_load_\w+ .*\blds\b)")
_VM_LOAD = re.compile(r"^(global|buffer|flat|scratch)_load_\w+\b")  # direct-to-LDS or not


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    pytest.skip("hipcc not available")


def _ring_depth() -> int:
    m = re.search(r"^#define LLFE_ST_LDSQ (\d+)", open(SRC).read(), re.M)
    assert m, "LLFE_ST_LDSQ's default not found in stencil_stream.hip"
    return int(m.group(1))


def _function(asm: str, mangled_part: str) -> str:
    m = re.search(r"^(_Z\S*" + mangled_part + r"\S*):", asm, re.M)
    assert m, f"{mangled_part} not in the ISA"
    end = re.compile(r"^\.Lfunc_end\d+:", re.M).search(asm, m.end())
    assert end, f"{mangled_part}: no end of function"
    return asm[m.end():end.start()]


def _blocks(body: str):
    """Basic blocks of a function's text: ([instructions], [successor block indices]) each.  A
    block starts at the entry, at a label and after a branch; s_branch goes to its target,
    s_cbranch_* to its target and on, everything else but s_endpgm falls through."""
    blocks, labels, cur = [], {}, []
    for ln in body.splitlines():
        s = ln.split(";")[0].strip()
        if not s:
            continue
        m = _LABEL.match(s)
        if m:
            if cur:
                blocks.append(cur)
                cur = []
            labels[m.group(1)] = len(blocks)  # (several labels may name one block)
            continue
        if s.startswith("."):  # directives
            continue
        assert not re.match(r"s_(setpc|swappc|call)", s), f"indirect control flow in the kernel: {s}"
        cur.append(s)
        if _BRANCH.match(s) or s.startswith("s_endpgm"):
            blocks.append(cur)
            cur = []
    if cur:
        blocks.append(cur)
    succ = []
    for i, b in enumerate(blocks):
        m = _BRANCH.match(b[-1])
        out = []
        if m:
            assert m.group(2) in labels, f"branch to an unknown label: {b[-1]}"
            out.append(labels[m.group(2)])
        if not (m and m.group(1) == "branch") and not b[-1].startswith("s_endpgm") and i + 1 < len(blocks):
            out.append(i + 1)
        succ.append(out)
    return blocks, succ


def _walk_back(blocks, preds, b, i, classify):
    """Walks backwards from instruction i of block b (exclusive) along every path.  classify(ins,
    block, index) ends a path by returning a verdict, or returns None to go on; a path that
    reaches the function's entry ends with "entry".  Returns the set of verdicts."""
    verdicts, seen, todo = set(), set(), [(b, i)]
    while todo:
        b, i = todo.pop()
        for j in range(i - 1, -1, -1):
            v = classify(blocks[b][j], b, j)
            if v is not None:
                verdicts.add(v)
                break
        else:
            if b == 0:
                verdicts.add("entry")
            for p in preds[b]:
                if p not in seen:
                    seen.add(p)
                    todo.append((p, len(blocks[p])))
    return verdicts


def ring_wait_faults(body: str, depth: int):
    """Checks the rules of this module's docstring on one function's text.  Returns (faults,
    leaders): the violations as strings, and the number of reads that open a step's ring reads."""
    blocks, succ = _blocks(body)
    preds = [[] for _ in blocks]
    for i, out in enumerate(succ):
        for s in out:
            preds[s].append(i)

    def before_read(ins, b, j):
        if _RING_READ.match(ins):
            return "read"
        if _LDS_LOAD.match(ins):
            return "load with no wait"
        m = _VMWAIT.match(ins)
        if m:
            return ("wait", int(m.group(1)), b, j)
        return None

    def before_counted_wait(ins, b, j):
        if _LDS_LOAD.match(ins):
            return "load"
        if _RING_READ.match(ins):
            return "read"
        return None

    def before_drain(ins, b, j):
        if _VM_LOAD.match(ins):
            return "vm load"
        if _RING_READ.match(ins):
            return "read"
        return None

    faults, leaders = [], 0
    for b, blk in enumerate(blocks):
        for i, ins in enumerate(blk):
            if not _RING_READ.match(ins):
                continue
            verdicts = _walk_back(blocks, preds, b, i, before_read)
            if "load with no wait" in verdicts:
                faults.append(f"`{ins}`: a path issues a direct-to-LDS load and reads the ring with no vmcnt wait")
            own_drain = counted = False
            for v in verdicts:
                if not isinstance(v, tuple):
                    continue
                _, n, wb, wi = v
                if n == 0:
                    # the kernel's own drain, not a wait of the compiler's behind ordinary loads
                    own_drain |= bool(_walk_back(blocks, preds, wb, wi, before_drain) & {"read", "entry"})
                    continue
                if n > depth - 2:
                    faults.append(f"`{ins}`: waits with vmcnt({n}), more than QD - 2 = {depth - 2}")
                    continue
                into = _walk_back(blocks, preds, wb, wi, before_counted_wait)
                if into != {"load"}:
                    faults.append(f"`{ins}`: a path reaches its vmcnt({n}) wait without this step's direct-to-LDS "
                                  f"load (from: {sorted(into - {'load'})}): the count is not there, the wait must drain")
                else:
                    counted = True
            if any(_RING_READ.match(x) for x in blk[:i]):
                continue  # a later read of the same gather: the first one stands for it
            leaders += 1
            if not own_drain:
                faults.append(f"`{ins}`: no path in front of it holds a vmcnt(0) of the kernel's own (one that no "
                              f"vector-memory load of the step precedes): the tail reads with no drain")
            if not counted:
                faults.append(f"`{ins}`: no path in front of it holds a counted wait behind the step's own load")
    return faults, leaders


@pytest.fixture(scope="session")
def stencil_isa(tmp_path_factory):
    from low_level_feature_extraction_amd import _build
    out = tmp_path_factory.mktemp("stencil_isa") / "stencil_stream.s"
    cmd = [_hipcc(), *_build.compile_flags("stencil_stream.hip"), "--cuda-device-only", "-S", SRC, "-o", str(out)]
    subprocess.run(cmd, check=True, capture_output=True, timeout=600)
    return out.read_text()


@pytest.mark.parametrize("kernel", KERNELS)
def test_stencil_ring_reads_wait_for_their_rows(stencil_isa, kernel):
    body = _function(stencil_isa, kernel)
    lines = [ln.split(";")[0].strip() for ln in body.splitlines()]
    assert sum("global_load_lds_dwordx3" in ln for ln in lines) >= 12, "interior rows: direct-to-LDS loads"
    assert sum(re.search(r"buffer_load_dwordx3 .* lds", ln) is not None for ln in lines) >= 12, \
        "border rows: range-checked buffer loads to LDS"
    assert sum(_INTERIOR_READ.match(ln) is not None for ln in lines) >= 12, "one ring read per unrolled row step"
    assert sum(_RING_READ.match(ln) is not None and _INTERIOR_READ.match(ln) is None for ln in lines) >= 12, \
        "border waves gather their REFLECT_101 columns from the ring row"
    faults, leaders = ring_wait_faults(body, _ring_depth())
    assert not faults, f"{kernel}: {len(faults)} ring reads are not guarded by count:\n" + "\n".join(faults[:8])
    assert leaders >= 24, "an interior read and a border gather per unrolled row step, each checked for both waits"


# The checker on hand-written functions: one row step of each shape, in a loop.
_STEP_HEAD = """
_Z4stepv:
    s_cbranch_scc1 .LBB0_9
.LBB0_1:
    s_cbranch_vccnz .LBB0_3
    global_load_lds_dwordx3 v[0:1], off
"""
_STEP_TAIL = """
    ds_read_b96 v[2:4], v5
    s_cbranch_scc0 .LBB0_1
.LBB0_9:
    s_endpgm
.Lfunc_end0:
"""
_BYTE_ARM = " s_cbranch_vccz .LBB0_5\n flat_load_ubyte v6, v[0:1]\n s_waitcnt vmcnt(0) lgkmcnt(0)\n ds_write_b96 v5, v[6:8]\n.LBB0_5:\n"
_SHAPES = {
    # the wait after the join of the load's arm and the arm without it: a count that is not there
    "joined": (_STEP_HEAD + ".LBB0_3:\n s_waitcnt vmcnt(4)\n" + _STEP_TAIL, False),
    # the counted wait in the load's arm and no wait in the other: the tail reads with no drain
    "arm": (_STEP_HEAD + " s_waitcnt vmcnt(4)\n.LBB0_3:\n" + _STEP_TAIL, False),
    "arm_and_drain": (_STEP_HEAD + " s_waitcnt vmcnt(4)\n s_branch .LBB0_4\n.LBB0_3:\n s_waitcnt vmcnt(0)\n.LBB0_4:\n" + _STEP_TAIL, True),
    # the same with a byte arm whose ordinary loads the compiler waits for itself
    "arm_byte_arm_and_drain": (_STEP_HEAD + " s_waitcnt vmcnt(4)\n s_branch .LBB0_4\n.LBB0_3:\n" + _BYTE_ARM
                               + " s_cbranch_scc1 .LBB0_4\n s_waitcnt vmcnt(0)\n.LBB0_4:\n" + _STEP_TAIL, True),
    # ... and without the tail's drain: the compiler's vmcnt(0) in the byte arm does not stand in for it
    "arm_byte_arm_no_drain": (_STEP_HEAD + " s_waitcnt vmcnt(4)\n s_branch .LBB0_4\n.LBB0_3:\n" + _BYTE_ARM
                              + ".LBB0_4:\n" + _STEP_TAIL, False),
    # a drain alone: the steady state would drain the ring every step
    "drain_only": (_STEP_HEAD + ".LBB0_3:\n s_waitcnt vmcnt(0)\n" + _STEP_TAIL, False),
    "arm_and_count": (_STEP_HEAD + " s_waitcnt vmcnt(4)\n s_branch .LBB0_4\n.LBB0_3:\n s_waitcnt vmcnt(3)\n.LBB0_4:\n" + _STEP_TAIL, False),
    "too_many": (_STEP_HEAD + " s_waitcnt vmcnt(5)\n s_branch .LBB0_4\n.LBB0_3:\n s_waitcnt vmcnt(0)\n.LBB0_4:\n" + _STEP_TAIL, False),
    "no_wait": (_STEP_HEAD + ".LBB0_3:\n" + _STEP_TAIL, False),
    "wait_above_load": (_STEP_HEAD.replace(" global_load", " s_waitcnt vmcnt(0)\n global_load") + ".LBB0_3:\n" + _STEP_TAIL, False),
}


@pytest.mark.parametrize("shape", sorted(_SHAPES))
def test_ring_wait_checker_on_handwritten_steps(shape):
    asm, good = _SHAPES[shape]
    faults, leaders = ring_wait_faults(_function(asm, "stepv"), 6)
    assert leaders == 1
    assert (not faults) == good, faults
