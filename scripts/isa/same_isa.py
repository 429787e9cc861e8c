#!/usr/bin/env python3
"""Refactoring gate: does the working tree compile to the same gfx950 ISA as revision REV?

Materialises REV's reacherdistilation_amd/csrc and include into a temporary directory (git
archive), compiles every .hip source of both trees with the hygiene tests' command line
(tests/test_product_hygiene.py product_isa: -O3 -std=c++17 --offload-arch -munsafe-fp-atomics plus
build.src_flags, --cuda-device-only -S) and prints per source `identical` or the functions whose
instruction text differs (hazards.functions).  Exits nonzero on any difference.  It compares text
only; it is not a test.  Sources named after REV restrict the run to them; --sha256 OUT.json also
records the sha256 of every .s of both trees.

usage: same_isa.py REV [SOURCE.hip ...] [--sha256 OUT.json]"""
import hashlib
import io
import json
import os
import subprocess
import sys
import tarfile
import tempfile
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import hazards as hz  # noqa: E402
from reacherdistilation_amd import build  # noqa: E402

CSRC = "reacherdistilation_amd/csrc"


def compile_tree(root, out, only):
    """{source: path of its .s} for every .hip under root/CSRC (flags by the source's base name)."""
    os.makedirs(out, exist_ok=True)
    srcs = sorted(f for f in os.listdir(os.path.join(root, CSRC)) if f.endswith(".hip") and (not only or f in only))

    def cc(f):
        s = os.path.join(out, f[:-4] + ".s")
        r = subprocess.run([build.HIPCC, "-O3", "-std=c++17", f"--offload-arch={build.ARCH}", "-munsafe-fp-atomics",
                            *build.src_flags(f), "-Wno-unused-command-line-argument", "--cuda-device-only", "-S",
                            # the one addition: hipcc names a __hip_cuid_<hash of the source's path> symbol,
                            # which would differ between the two trees; pinned, the .s files compare bytewise
                            f"-cuid={f}", "-o", s, os.path.join(root, CSRC, f)], capture_output=True, text=True)
        if r.returncode:
            sys.exit(f"{root}: {f} does not compile\n{r.stderr}")
        return f, s

    with ThreadPoolExecutor(min(len(srcs), 16)) as ex:
        return dict(ex.map(cc, srcs))


def sha256(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()


def main():
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    rev = sys.argv[1]
    sha_out = sys.argv[sys.argv.index("--sha256") + 1] if "--sha256" in sys.argv else None
    only = [a for a in sys.argv[2:] if a.endswith(".hip")]
    with tempfile.TemporaryDirectory() as tmp:
        tar = subprocess.run(["git", "-C", ROOT, "archive", rev, CSRC, "include"], check=True, capture_output=True).stdout
        tarfile.open(fileobj=io.BytesIO(tar)).extractall(os.path.join(tmp, "old"))
        old = compile_tree(os.path.join(tmp, "old"), os.path.join(tmp, "old_s"), only)
        new = compile_tree(ROOT, os.path.join(tmp, "new_s"), only)
        differ = False
        shas = {}
        for f in sorted(set(old) | set(new)):
            if f not in old or f not in new:
                print(f"{f}: only in {'the working tree' if f in new else rev}")
                differ = True
                continue
            shas[f] = {"parent": sha256(old[f]), "new": sha256(new[f])}
            if shas[f]["parent"] == shas[f]["new"]:
                print(f"{f}: identical")
                continue
            differ = True
            a, b = hz.functions(old[f]), hz.functions(new[f])
            text = lambda code: [l for _, l in code]  # noqa: E731
            names = [n for n in sorted(set(a) | set(b)) if n not in a or n not in b or text(a[n]) != text(b[n])]
            if names or list(a) != list(b):
                print(f"{f}: {len(names)} of {len(b)} functions differ" + ("" if list(a) == list(b) else " (and their order)"))
            else:
                print(f"{f}: same instructions, other text differs (directives, metadata or comments)")
            for n in names:
                print(f"    {n}")
        if sha_out:
            rev_id = subprocess.run(["git", "-C", ROOT, "rev-parse", rev], check=True, capture_output=True, text=True).stdout.strip()
            json.dump({"parent_rev": rev_id, "arch": build.ARCH, "sources": shas}, open(sha_out, "w"), indent=1)
            open(sha_out, "a").write("\n")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
