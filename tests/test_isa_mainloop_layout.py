"""ISA-level guard for the schedule of the split engine's main loop (csrc/bf3_engine.hpp; runs without a GPU).

An LDS-DMA piece (`buffer_load_dwordx4 ... lds`) that is issued late in a stage and retired by the wait in front of the next
barrier has no time to land: all eight waves of the workgroup then stand at that barrier until the slowest piece has come in
from wherever it lives.  The loop is written so that EVERY piece has at least one full stage of its own wave's MFMAs between
its issue and the `s_waitcnt vmcnt(N)` that retires it -- 48 `v_mfma_f32_16x16x32_f16` for the two-plane fp16 scheme, 96
`v_mfma_f32_16x16x32_bf16` for the three-plane bf16 scheme.  The compiler is free to move vector-memory instructions among
MFMAs, so this is checked on what it emitted: the test disassembles the built library, takes every innermost loop body that
holds both instructions, replays the vmcnt queue (vector-memory operations retire in issue order; `vmcnt(N)` waits until at
most N are outstanding) over consecutive trips of the body -- two for pieces retired within a stage, a third where the ring
retires them two stages later -- and counts, per piece issued in the first trip, the MFMAs up to its retiring wait.
"""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(os.path.dirname(HERE), "projected-lmc_amd", "projectedlmc", "libplmc_hip.so")
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"

FUNC = re.compile(r"^([0-9a-f]+) <(.+)>:")
INS = re.compile(r"^\s+([a-z]\S*)\s*(.*?)\s*//\s*([0-9A-Fa-f]+):\s*\S+(.*)$")
TARGET = re.compile(r"<.+\+0x([0-9a-f]+)>")
DMA = re.compile(r"^buffer_load_dwordx4\b.*\blds\b")
MFMA = re.compile(r"^v_mfma_f32_16x16x32_(f16|bf16)\b")
VMEM = re.compile(r"^(buffer|global|flat|scratch)_(load|store|atomic)")
VMCNT = re.compile(r"vmcnt\((\d+)\)")
STAGE_MFMAS = {"f16": 48, "bf16": 96}


def _functions():
    """{name: [(address, text)]} over every gfx950 code object of the library"""
    if not (os.path.exists(LIB) and os.path.exists(OBJDUMP)):
        pytest.skip("library or llvm-objdump not available")
    tmp = tempfile.mkdtemp(prefix="plmc_isa_")
    funcs = {}
    try:
        lib = shutil.copy(LIB, tmp)
        subprocess.run([OBJDUMP, "--offloading", lib], cwd=tmp, capture_output=True, check=True)
        for f in sorted(os.listdir(tmp)):
            if "amdgcn" not in f:
                continue
            out = subprocess.run([OBJDUMP, "-d", os.path.join(tmp, f)], capture_output=True, text=True, check=True).stdout
            cur, start = None, 0
            for raw in out.splitlines():
                m = FUNC.match(raw)
                if m:
                    start = int(m.group(1), 16)
                    cur = funcs.setdefault("%s:%s" % (f, m.group(2)), [])
                    continue
                m = INS.match(raw)
                if m and cur is not None:
                    text = (m.group(1) + " " + m.group(2)).strip()
                    target = None
                    if text.startswith("s_cbranch") or text.startswith("s_branch"):
                        t = TARGET.search(m.group(4))
                        target = start + int(t.group(1), 16) if t else None
                    cur.append((int(m.group(3), 16), text, target))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return funcs


def _loop_bodies(ins):
    """innermost loops of one function: instruction lists between a backward branch's target and the branch"""
    back = [(i, t) for i, (a, _, t) in enumerate(ins) if t is not None and t <= a]
    addr = {a: i for i, (a, _, _) in enumerate(ins)}
    bodies = []
    for i, t in back:
        if t not in addr:
            continue
        lo = addr[t]
        if any(lo <= j < i for j, _ in back):                    # holds another loop: not innermost
            continue
        bodies.append([text for _, text, _ in ins[lo:i + 1]])
    return bodies


def _min_mfmas_to_retire(body, trips=3):
    """replay: per DMA piece issued in the first trip, MFMAs between its issue and the wait that retires it (a piece that is
    still in flight after `trips` trips counts what it has seen)"""
    queue, mfmas, gaps = [], 0, []
    for trip in range(trips):
        for text in body:
            if MFMA.match(text):
                mfmas += 1
            elif VMEM.match(text):
                queue.append((trip == 0 and bool(DMA.match(text)), mfmas))
            elif text.startswith("s_waitcnt"):
                m = VMCNT.search(text)
                if m:
                    while len(queue) > int(m.group(1)):
                        first_trip_piece, at = queue.pop(0)
                        if first_trip_piece:
                            gaps.append(mfmas - at)
    gaps += [mfmas - at for first_trip_piece, at in queue if first_trip_piece]
    return min(gaps), sorted(gaps)


def test_every_dma_piece_has_a_stage_of_mfmas_before_its_wait():
    seen, bad = {"f16": 0, "bf16": 0}, []
    for name, ins in _functions().items():
        for body in _loop_bodies(ins):
            kinds = {MFMA.match(t).group(1) for t in body if MFMA.match(t)}
            if not kinds or not any(DMA.match(t) for t in body):
                continue
            assert len(kinds) == 1, (name, kinds)
            kind = kinds.pop()
            seen[kind] += 1
            least, gaps = _min_mfmas_to_retire(body)
            if least < STAGE_MFMAS[kind]:
                bad.append((name.split(":")[-1], kind, least, gaps))
    assert seen["f16"] >= 4 and seen["bf16"] >= 4, "the scan is not looking at the split-engine kernels: %r" % seen
    assert not bad, "%d of %d main loops retire a DMA piece after fewer MFMAs than one stage: %r" % (len(bad), sum(seen.values()), bad[:6])
