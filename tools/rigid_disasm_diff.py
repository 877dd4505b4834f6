"""Compare the gfx950 kernels of two builds of the library instruction by instruction.

    python tools/rigid_disasm_diff.py OLD.so NEW.so [--show N]

Every kernel symbol of OLD is disassembled in both libraries (llvm-objdump, no addresses, no encodings; branch targets and
PC-relative constants reduced to placeholders) and the instruction lists are compared.  Prints how many are identical,
which differ (by family), which are missing from NEW and which are new in NEW.  Used to show that adding the scaled kernels
left every rigid kernel as it was (CHANGELOG.md).
"""
import collections
import difflib
import importlib.util
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tests", "test_kernel_resources.py"))
kr = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(kr)


def functions(lib):
    out = {}
    for co in kr.code_objects(lib):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(co)
            f.flush()
            txt = subprocess.run([kr._tool("llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", f.name],
                                 check=True, stdout=subprocess.PIPE).stdout.decode()
        cur = None
        for line in txt.splitlines():
            m = re.match(r"^(?:[0-9a-f]+ )?<(.+)>:$", line)
            if m:
                cur = m.group(1)
                out.setdefault(cur, [])
                continue
            if cur is None or not line.strip():
                continue
            line = re.sub(r"//.*$", "", line).rstrip()
            if "s_getpc" in line or "branch" in line:
                line = re.sub(r"0x[0-9a-f]+", "ADDR", line)
            out[cur].append(re.sub(r"<[^>]*>", "<L>", line).strip())
    return out


def family(sym):
    m = re.search(r"(k_\w+?)(?:I|E)", sym)
    return m.group(1) if m else sym[:40]


def main():
    old, new = functions(sys.argv[1]), functions(sys.argv[2])
    show = int(sys.argv[sys.argv.index("--show") + 1]) if "--show" in sys.argv else 0
    diff = [k for k in old if k in new and old[k] != new[k]]
    missing = [k for k in old if k not in new]
    added = [k for k in new if k not in old]
    print(f"kernels in {os.path.basename(sys.argv[1])}: {len(old)}; identical: {len(old) - len(diff) - len(missing)}; "
          f"differing: {len(diff)}; missing: {len(missing)}; new: {len(added)}")
    print("differing by family:", dict(collections.Counter(family(k) for k in diff)))
    print("new by family:", dict(collections.Counter(family(k) for k in added)))
    for k in diff[:show]:
        d = [l for l in difflib.unified_diff(old[k], new[k], lineterm="", n=0) if l[:1] in "+-" and l[:3] not in ("+++", "---")]
        print(f"{k}: {len(d)} lines differ")
        print("\n".join(d[:12]))


if __name__ == "__main__":
    main()
