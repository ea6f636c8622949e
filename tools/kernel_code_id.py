#!/usr/bin/env python3
"""Identity of a kernel symbol's MACHINE CODE in a built library: sha256 over the symbol's disassembled instructions
(mnemonics and operands, no addresses). A PMC traffic figure recorded in profiles/pmc_traffic.json belongs to the machine
code it was measured on; an edit elsewhere in the kernel's source (another template instantiation) changes the source id
but not that code - bench.py accepts a recorded figure when either matches. kernel_source_files() / kernel_source_id_full():
the kernel's source over ALL its files (search_kernel.inc's parts included), which is what the tools record.
usage: kernel_code_id.py [library] [regex over demangled names] [kernel name]   -> one line per symbol
The kernel name (default seismic_search_kernel) picks the function template whose instances are looked at; the library
may also be a bare code object (hipcc --offload-device-only --no-gpu-bundle-output), which needs no link:
  kernel_code_id.py build/score_documents.co "" score_documents_kernel"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import check_coop_asm as cca  # noqa: E402


def code_ids(lib=None, pattern=None, kernel="seismic_search_kernel"):
    """{demangled symbol (template arguments only; "" for a kernel that is no template): 16 hex digits} for the symbols of
    `kernel` in namespace sgpu (or an unnamed one inside it) whose demangled name matches `pattern`."""
    lib = lib or os.environ.get("SGPU_LIB") or os.path.join(cca.ROOT, "seismic_amd", "libseismic_hip.so")
    rx, out = re.compile(pattern or (kernel + r"\b")), {}
    mangled = re.compile(r"^_ZN4sgpu(?:12_GLOBAL__N_1)?%d%s" % (len(kernel), kernel))
    with tempfile.TemporaryDirectory() as td:
        for k, co in enumerate(cca.code_objects(lib) or [open(lib, "rb").read()]):
            path = os.path.join(td, "co%d.o" % k)
            open(path, "wb").write(co)
            syms = subprocess.run([cca.LLVM + "/llvm-readelf", "-s", "-W", path], capture_output=True, text=True).stdout.split("\n")
            names = sorted({l.split()[-1] for l in syms if l.strip() and " FUNC " in l and mangled.match(l.split()[-1])})
            if not names:
                continue
            dem = subprocess.run(["c++filt"] + names, capture_output=True, text=True).stdout.split("\n")
            pick = [(m, d) for m, d in zip(names, dem) if rx.search(d)]
            if not pick:
                continue
            asm = subprocess.run([cca.LLVM + "/llvm-objdump", "-d", "--no-show-raw-insn", "--disassemble-symbols=" + ",".join(m for m, _ in pick), path],
                                 capture_output=True, text=True).stdout
            cur, h = None, {}
            for l in asm.split("\n"):
                m = re.match(r"^[0-9a-f]+ <(\S+)>:", l)
                if m:
                    cur = m.group(1)
                    h[cur] = hashlib.sha256()
                elif cur and (l.startswith("\t") or l.startswith(" ")):
                    h[cur].update((l.split("//")[0].strip() + "\n").encode())
            for m, d in pick:
                if m in h:
                    out[re.search(kernel + r"(<.*?>)?\(", d).group(1) or ""] = h[m].hexdigest()[:16]
    return out


CSRC = os.path.join(cca.ROOT, "seismic_amd", "csrc")


def kernel_source_files():
    """Base names of the csrc files the search kernels are compiled from: the set bench.kernel_source_id() hashes
    (search_kernel.inc, device_types.hpp, sk_*.hip) and every csrc file search_kernel.inc includes in quotes, transitively
    (its search_*.inc parts, record.hpp, ...), sorted."""
    todo = ["search_kernel.inc", "device_types.hpp"] + [f for f in os.listdir(CSRC) if re.fullmatch(r"sk_\w+\.hip", f)]
    seen = set()
    while todo:
        f = todo.pop()
        if f in seen or not os.path.exists(os.path.join(CSRC, f)):
            continue
        seen.add(f)
        if f.startswith("sk_"):   # (the units only include search_kernel.inc)
            continue
        todo += re.findall(r'^\s*#\s*include\s+"([^"]+)"', open(os.path.join(CSRC, f)).read(), re.M)
    return sorted(seen)


def kernel_source_id_full():
    """Identity of the search kernels' whole source. bench.kernel_source_id() covers search_kernel.inc, device_types.hpp and
    the units only: an edit to an included part leaves it as it was. New entries of profiles/pmc_traffic.json carry this id
    instead, which bench's source comparison never matches - its machine-code comparison (symbol_code_id) decides."""
    h = hashlib.sha256()
    for f in kernel_source_files():
        h.update(f.encode() + b"\0" + open(os.path.join(CSRC, f), "rb").read())
    return h.hexdigest()[:16]


if __name__ == "__main__":
    ids = code_ids(sys.argv[1] if len(sys.argv) > 1 else None, sys.argv[2] if len(sys.argv) > 2 and sys.argv[2] else None,
                   sys.argv[3] if len(sys.argv) > 3 else "seismic_search_kernel")
    for k in sorted(ids):
        print(ids[k], k)
