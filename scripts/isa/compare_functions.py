"""Compare the instruction text of kernel functions between two builds of libreacher.so.

    python scripts/isa/compare_functions.py OLD.so NEW.so REGEX [REGEX ...] [--out report.txt]
                                            [--rename REGEX=REPL ...]

Both libraries' gfx950 code objects are extracted (llvm-objdump --offloading, on copies in a
temporary folder) and disassembled; every function whose DEMANGLED name matches one of the regular
expressions is compared.  A function's text is its instructions in order -- mnemonic and operands,
without addresses and encodings; branch targets, which objdump prints as addresses, are rewritten
relative to the function's start, so a function that only moved inside the object compares equal.
Functions are paired by demangled name.  A template that gained trailing defaulted parameters: where
NEW has no function of OLD's name, its partner is the one function of NEW whose template arguments
are OLD's followed by further ones none of which is `true` (the defaults of a new switch: false, a type).
A template that lost a parameter: --rename REGEX=REPL (re.sub) rewrites OLD's names before the pairing;
the report names both.
Exit status 1 if a paired function differs or a function of OLD has no partner.
"""
from __future__ import annotations

import argparse
import difflib
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.environ.get("RD_LLVM_BIN", "/opt/rocm/llvm/bin")


def code_objects(lib: str, tmp: str) -> list[str]:
    d = tempfile.mkdtemp(dir=tmp)
    copy = os.path.join(d, "lib.so")
    shutil.copy(lib, copy)
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", copy], check=True, capture_output=True)
    return sorted(os.path.join(d, f) for f in os.listdir(d) if "amdgcn" in f)


def functions(co: str) -> dict[str, list[str]]:
    """demangled name -> instruction text"""
    out = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--demangle", "--no-show-raw-insn", co],
                         check=True, capture_output=True, text=True).stdout
    fns: dict[str, list[str]] = {}
    cur, base = None, 0
    for ln in out.splitlines():
        m = re.match(r"^([0-9a-f]+) <(.*)>:$", ln)
        if m:
            base, cur = int(m.group(1), 16), []
            fns[m.group(2)] = cur
            continue
        if cur is None or not ln.startswith(" ") and not ln.startswith("\t"):
            continue
        txt = ln.split("//")[0].strip()
        if not txt:
            continue
        cm = re.search(r"//\s*([0-9A-Fa-f]+):", ln)
        # a branch's target: "s_cbranch_scc1 12345  // ...: <sym+0x40>" keeps the symbol-relative form
        tgt = re.search(r"<[^>]*\+0x([0-9a-f]+)>", ln)
        if tgt and re.match(r"s_(c?branch|call)", txt):
            txt = re.sub(r"\s\S+$", f" +0x{tgt.group(1)}", txt)
        elif re.match(r"s_c?branch", txt) and cm:
            off = int(txt.split()[-1])
            here = int(cm.group(1), 16)
            txt = re.sub(r"\s\S+$", f" +0x{here + 4 + 4 * off - base:x}", txt)
        cur.append(txt)
    return fns


def partner_of(name: str, new: dict) -> str | None:
    if name in new:
        return name
    m = re.match(r"^(.*<.*)(>\(.*)$", name)
    if not m:
        return None
    cands = [n for n in new if n.startswith(m.group(1) + ", ") and n.endswith(m.group(2))
             and "true" not in n[len(m.group(1)):len(n) - len(m.group(2))]]
    return cands[0] if len(cands) == 1 else None


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("patterns", nargs="+")
    ap.add_argument("--out")
    ap.add_argument("--rename", action="append", default=[], metavar="REGEX=REPL")
    a = ap.parse_args()
    renames = [r.split("=", 1) for r in a.rename]
    tmp = tempfile.mkdtemp(prefix="rd_isa_")
    try:
        sides = []
        for lib in (a.old, a.new):
            fns: dict[str, list[str]] = {}
            for co in code_objects(lib, tmp):
                fns.update(functions(co))
            sides.append({n: c for n, c in fns.items() if any(re.search(p, n) for p in a.patterns)})
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    old, new = sides
    lines, bad = [], 0
    paired = set()
    for name in sorted(old):
        renamed = name
        for pat, repl in renames:
            renamed = re.sub(pat, repl, renamed)
        partner = partner_of(renamed, new)
        if partner is None:
            lines.append(f"MISSING   {name}")
            bad += 1
            continue
        paired.add(partner)
        same = old[name] == new[partner]
        tag = "identical" if same else "DIFFERS  "
        lines.append(f"{tag} {len(old[name]):6d} -> {len(new[partner]):6d} instructions  {name}"
                     + (f"  ->  {partner}" if partner != name else ""))
        if not same:
            bad += 1
            lines += ["    " + d for d in list(difflib.unified_diff(old[name], new[partner], lineterm="", n=1))[:40]]
    for name in sorted(set(new) - paired):
        lines.append(f"new       {len(new[name]):6d} instructions  {name}")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
