"""The cooperative reset's register invariant, checked on the compiler's output (csrc/skyjo_record.h: CoopRegs).

    python tools/check_coop_regs.py [file.s]

Without an argument the environment unit is compiled to assembly with the flags of skyjo_rl_amd/build.py (device side only).  In
every function that holds the cooperative pair, the four marker lines - `; coop reserve | request | commit | release` - must name the
same registers for the piece (d) and its LDS address (a), reserve and request the same scratch register (t), and between reserve and
release no instruction outside the request statement may write d or a (between reserve and request: t).  A copy or a re-use in
there would move or destroy only the lanes that were switched on at that point, while the statements work on other lanes' parts.

Limits.  The scan follows the function in LAYOUT order from the reserve marker to the release marker.  Blocks of the loop that the
compiler lays out behind the release (rare paths: the LDS-DMA of the games beyond the group, in-place deals) are not covered - some
of them run after the commit and re-use the registers rightly, so they cannot be told apart without the control flow; the compiler's
own liveness, which the reserve / release pair extends over the whole iteration, is what holds there.  Only VGPR destinations are
looked at: scalar instructions (`s_*`), stores, LDS writes, compares and lane reads name no VGPR they write as their first operand.
"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_WRITE = ("ds_write", "ds_add", "ds_sub", "ds_inc", "ds_max", "ds_min", "ds_or", "ds_and", "global_store", "buffer_store", "flat_store", "scratch_store",
            "global_atomic", "v_cmp", "v_readlane", "v_readfirstlane", "s_", "ds_gws", "ds_nop")


def regs(tok):
    m = re.fullmatch(r"v\[(\d+):(\d+)\]", tok)
    if m:
        return set(range(int(m.group(1)), int(m.group(2)) + 1))
    m = re.fullmatch(r"v(\d+)", tok)
    return {int(m.group(1))} if m else set()


def compile_unit():
    sys.path.insert(0, ROOT)
    from skyjo_rl_amd import build
    out = os.path.join(tempfile.mkdtemp(prefix="coop_regs_"), "skyjo_capi.s")
    name, src, unit_flags = build.UNITS[0]
    flags = [f for f in build.FLAGS if f != "-fPIC"]
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + flags + list(unit_flags) + ["--cuda-device-only", "-S", "-o", out, src])
    return out


def check(path):
    """-> (number of functions that hold the pair, list of violations)"""
    bad, found = [], 0
    func, state, marks, in_asm, asm_is_request = None, None, {}, False, False
    for n, line in enumerate(open(path), 1):
        t = line.strip()
        if line[:1] not in " \t.;\n" and t.endswith(":") or re.match(r"^_Z\w+:", line):
            func, state, marks = t.split(":")[0], None, {}
        m = re.match(r"; coop (reserve|request|commit|release) (\S+) (\S+)(?: (\S+))?", t)
        if m:
            kind = m.group(1)
            marks[kind] = (regs(m.group(2)), regs(m.group(3)), regs(m.group(4) or ""))
            if kind == "reserve":
                found += 1
                state = "to_request"
            elif kind == "request":
                if marks[kind] != marks.get("reserve"):
                    bad.append(f"{path}:{n}: {func}: the request names other registers than the reserve: {t}")
                state, asm_is_request = "to_release", True
            else:
                r = marks.get("reserve")
                if not r or marks[kind][:2] != r[:2]:
                    bad.append(f"{path}:{n}: {func}: the {kind} names other registers than the reserve: {t}")
                if kind == "release":
                    state = None
            continue
        if t.startswith(";;#ASMSTART"):
            in_asm = True
            continue
        if t.startswith(";;#ASMEND"):
            in_asm, asm_is_request = False, False
            continue
        if state is None or not t or t[0] in ";." or t.endswith(":"):
            continue
        if in_asm and asm_is_request:
            continue  # the request statement itself
        parts = t.split(None, 1)
        if len(parts) < 2 or parts[0].startswith(NO_WRITE):
            continue
        dst = regs(parts[1].split(",")[0].strip())
        d, a, tt = marks["reserve"]
        guarded = d | a | (tt if state == "to_request" else set())
        if dst & guarded:
            bad.append(f"{path}:{n}: {func}: writes a reserved register between reserve and release: {t}")
    return found, bad


if __name__ == "__main__":
    p = sys.argv[1] if len(sys.argv) > 1 else compile_unit()
    found, bad = check(p)
    print(f"{found} functions hold the cooperative pair, {len(bad)} violations")
    for b in bad:
        print(b)
    sys.exit(1 if bad or not found else 0)
