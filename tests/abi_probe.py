"""The header against the ctypes binding, by compiler (helper of tests/test_capi_signatures.py).

From a signature table (name -> (restype, argtypes)), a set of ctypes structures and a list of constants this module
writes ONE C++17 program that includes include/skyjo_vec.h and prints, for every name, what the C++ compiler makes of the
header: a prototype as a string of type tokens taken from decltype(function) by parameter-pack matching, offsetof / field
size / sizeof by field name, and the value of every #define.  Nothing is parsed with a regular expression and nothing is
linked: the program only inspects types.  The same strings are built from the ctypes side and the two are compared.

Tokens: `P` any pointer or decayed array, `i<n>` / `u<n>` a signed / unsigned integer of n bytes, `f<n>` a floating type of
n bytes, `v` void.  A prototype reads `ret(arg,arg,...)`.
"""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")

# ctypes structure of skyjo_rl_amd._lib -> the header's struct
STRUCTS = {
    "Config": "skyjo_vec_config",
    "Info": "skyjo_vec_info",
    "Counters": "skyjo_vec_counters",
    "GameState": "skyjo_game_state",
    "RolloutBuffers": "skyjo_vec_rollout_buffers",
    "SeatPolicy": "skyjo_vec_seat_policy",
    "PPOUpdateArgs": "skyjo_vec_ppo_update_args",
}

# name in skyjo_rl_amd._lib -> the header's #define.  mirrored_names() finds what _lib holds; a name missing here fails the test.
CONSTANTS = {
    "ABI_VERSION": "SKYJO_ABI_VERSION", "MAX_PLAYERS": "SKYJO_MAX_PLAYERS",
    "ST_OK": "SKYJO_ST_OK", "ST_ILLEGAL": "SKYJO_ST_ILLEGAL", "ST_NOOP_DONE": "SKYJO_ST_NOOP_DONE",
    "ST_RESET": "SKYJO_ST_RESET", "ST_ERROR": "SKYJO_ST_ERROR",
    "RNG_MT19937": "SKYJO_RNG_MT19937", "RNG_PHILOX": "SKYJO_RNG_PHILOX",
    "MLP_BF16": "SKYJO_MLP_BF16", "MLP_FP32": "SKYJO_MLP_FP32",
    "ACTION_SKIP": "SKYJO_ACTION_SKIP",
    "OPT_RECORD_LAYOUT": "SKYJO_OPT_RECORD_LAYOUT", "OPT_INLINE_WORK_LIST": "SKYJO_OPT_INLINE_WORK_LIST",
    "OPT_UNPIPELINED": "SKYJO_OPT_UNPIPELINED", "OPT_CYCLE_S": "SKYJO_OPT_CYCLE_S",
    "OPT_MAX_CYCLES_PER_LAUNCH": "SKYJO_OPT_MAX_CYCLES_PER_LAUNCH",
    "REC_ROW_MAJOR": "SKYJO_REC_ROW_MAJOR", "REC_TILE_PLANAR": "SKYJO_REC_TILE_PLANAR",
    "REC_TILE_PLANAR_ALL": "SKYJO_REC_TILE_PLANAR_ALL",
    "TGT_HAS_TARGET": "SKYJO_TGT_HAS_TARGET", "TGT_EPISODE_KNOWN": "SKYJO_TGT_EPISODE_KNOWN",
    "SEAT_SAMPLE": "SKYJO_SEAT_SAMPLE", "SEAT_GREEDY": "SKYJO_SEAT_GREEDY", "SEAT_RANDOM": "SKYJO_SEAT_RANDOM",
    "UPDATE_STATS": "SKYJO_UPDATE_STATS", "E_INVALID": "SKYJO_E_INVALID",
}
# len(_lib.PROF_KERNELS) is held to this one
PROF_KERNELS_DEFINE = "SKYJO_PROF_KERNELS"


def mirrored_names(module):
    """Every module-level integer of `module` whose name is written in capitals: the header constants it restates."""
    return sorted(n for n, v in vars(module).items()
                  if re.fullmatch(r"[A-Z][A-Z0-9_]*", n) and isinstance(v, int) and not isinstance(v, bool))


_INT_CODES = "bhilq"


def token(ctype):
    """The type token of one ctypes restype / argtype (None is void)."""
    if ctype is None:
        return "v"
    if ctype in (C.c_void_p, C.c_char_p, C.c_wchar_p) or issubclass(ctype, (C._Pointer, C.Array)):
        return "P"
    code = getattr(ctype, "_type_", None)
    if isinstance(code, str) and len(code) == 1:
        if code in "fdg":
            return f"f{C.sizeof(ctype)}"
        if code.lower() in _INT_CODES:
            return ("i" if code in _INT_CODES else "u") + str(C.sizeof(ctype))
        if code in "PzZ":
            return "P"
    raise TypeError(f"no token for {ctype!r}")


def signature_string(restype, argtypes):
    return token(restype) + "(" + ",".join(token(a) for a in argtypes) + ")"


_PRELUDE = r"""
#include <cstddef>
#include <cstdio>
#include <string>
#include <type_traits>
#include "skyjo_vec.h"

template <class T> std::string tok() {
  using U = std::decay_t<T>;
  if constexpr (std::is_void_v<U>) return "v";
  else if constexpr (std::is_pointer_v<U>) return "P";
  else if constexpr (std::is_floating_point_v<U>) return "f" + std::to_string(sizeof(U));
  else if constexpr (std::is_integral_v<U>) return (std::is_signed_v<U> ? "i" : "u") + std::to_string(sizeof(U));
  else return "?";
}
template <class F> struct Sig;
template <class R, class... A> struct Sig<R(A...)> {
  static std::string str() {
    std::string s = tok<R>() + "(";
    bool first = true;
    ((s += (first ? "" : ",") + tok<A>(), first = false), ...);
    return s + ")";
  }
};
"""


def generate(signatures, structs=None, constants=None):
    """The probe's source.  signatures: iterable of function names; structs: {label: (header struct, [field names])};
    constants: {label: header #define}."""
    out = [_PRELUDE, "int main() {"]
    for name in signatures:
        out.append(f'  std::printf("F {name} %s\\n", Sig<decltype({name})>::str().c_str());')
    for label, (cname, fields) in (structs or {}).items():
        out.append(f'  std::printf("Z {label} %zu\\n", sizeof({cname}));')
        for f in fields:
            out.append(f'  std::printf("S {label} {f} %zu %zu\\n", offsetof({cname}, {f}), sizeof({cname}::{f}));')
    for label, define in (constants or {}).items():
        out.append(f'  std::printf("C {label} %lld\\n", (long long)({define}));')
    out.append("  return 0;\n}\n")
    return "\n".join(out)


class Probe:
    def __init__(self):
        self.functions, self.sizes, self.fields, self.constants = {}, {}, {}, {}


def run(source, workdir):
    """Compile the probe with g++ -std=c++17 -I include, run it, parse what it prints.  A compile error raises
    subprocess.CalledProcessError with the compiler's message in .stderr."""
    src, exe = os.path.join(str(workdir), "probe.cpp"), os.path.join(str(workdir), "probe")
    with open(src, "w") as f:
        f.write(source)
    subprocess.run(["g++", "-std=c++17", "-I", INCLUDE, src, "-o", exe], check=True, capture_output=True, text=True)
    p = Probe()
    for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines():
        w = line.split()
        if w[0] == "F":
            p.functions[w[1]] = w[2]
        elif w[0] == "Z":
            p.sizes[w[1]] = int(w[2])
        elif w[0] == "S":
            p.fields[(w[1], w[2])] = (int(w[3]), int(w[4]))
        elif w[0] == "C":
            p.constants[w[1]] = int(w[2])
    return p


def struct_spec(classes):
    """{label: (header struct, field names)} for ctypes classes given as {label: class}."""
    return {label: (STRUCTS[label], [f[0] for f in cls._fields_]) for label, cls in classes.items()}


def signature_mismatches(probe, table):
    """One line per function of `table` whose ctypes entry does not spell the header's prototype."""
    bad = []
    for name, (res, args) in table.items():
        want, got = probe.functions.get(name), signature_string(res, args)
        if want != got:
            bad.append(f"{name}: header {want}, binding {got}")
    return bad


def struct_mismatches(probe, classes):
    """One line per field (or whole size) of the ctypes classes {label: class} that the header lays out differently."""
    bad = []
    for label, cls in classes.items():
        if probe.sizes[label] != C.sizeof(cls):
            bad.append(f"{label}: sizeof {probe.sizes[label]} in the header, {C.sizeof(cls)} in ctypes")
        for f in cls._fields_:
            d = getattr(cls, f[0])
            if probe.fields[(label, f[0])] != (d.offset, d.size):
                bad.append(f"{label}.{f[0]}: (offset, size) {probe.fields[(label, f[0])]} in the header, {(d.offset, d.size)} in ctypes")
    return bad


def integration_config_fields(path=os.path.join(ROOT, "INTEGRATION.md")):
    """_fields_ of the `_Config` block of INTEGRATION.md section 2, evaluated with ctypes alone."""
    text = open(path).read()
    start = text.index("class _Config(C.Structure)")
    lines = text[start:].splitlines()
    block = [lines[0]]
    for line in lines[1:]:
        if line.strip() and not line.startswith(" "):
            break
        block.append(line)
    scope = {"C": C, "__builtins__": {"__build_class__": __build_class__, "__name__": "integration"}}
    exec("\n".join(block), scope)
    return scope["_Config"]._fields_
