"""Record the declaration hash of include/recalgo.h for its CURRENT RECALGO_ABI_VERSION in include/recalgo.abi — with
--cgc: of include/recalgo_cgc.h for its RECALGO_CGC_ABI_VERSION in include/recalgo_cgc.abi; with --wide: of
include/recalgo_wide.h for its RECALGO_WIDE_ABI_VERSION in include/recalgo_wide.abi; with --bst: of include/recalgo_bst.h
for its RECALGO_BST_ABI_VERSION in include/recalgo_bst.abi.
Run after bumping the version for a signature change (tests/test_abi.py / tests/test_ple_host.py / tests/test_wdl_host.py /
tests/test_bst_host.py compare).  Re-recording an
existing version is only legitimate while that version has not left the development tree (no library of it exists anywhere
else)."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
if "--cgc" in sys.argv[1:]:
    from tests.test_ple_host import HEADER, declaration_hash  # noqa: E402
    define, record = "RECALGO_CGC_ABI_VERSION", "recalgo_cgc.abi"
elif "--wide" in sys.argv[1:]:
    from tests.test_wdl_host import HEADER, declaration_hash  # noqa: E402
    define, record = "RECALGO_WIDE_ABI_VERSION", "recalgo_wide.abi"
elif "--bst" in sys.argv[1:]:
    from tests.test_bst_host import HEADER, declaration_hash  # noqa: E402
    define, record = "RECALGO_BST_ABI_VERSION", "recalgo_bst.abi"
else:
    from tests.test_abi import HEADER, declaration_hash  # noqa: E402
    define, record = "RECALGO_ABI_VERSION", "recalgo.abi"

version = int(re.search(rf"#define {define} (\d+)", open(HEADER).read()).group(1))
path = os.path.join(ROOT, "include", record)
lines = [ln for ln in open(path).read().splitlines() if ln.strip()] if os.path.exists(path) else []
lines = [ln for ln in lines if ln.startswith("#") or int(ln.split()[0]) != version]
lines.append(f"{version} {declaration_hash()}")
open(path, "w").write("\n".join(lines) + "\n")
print(lines[-1])
