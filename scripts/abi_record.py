"""python scripts/abi_record.py [HEADER]: record the declaration hash of include/HEADER (one of recalgorithm_amd._lib.HEADERS
_lib.MORE_HEADERS or _lib.SERVING_HEADERS, default recalgo.h) for its CURRENT ABI version in include/<stem>.abi.  Run after bumping the header's
version for a signature change (tests/test_abi.py compares).  Only the current version's line is rewritten; re-recording an existing version is only
legitimate while that version has not left the development tree (no library of it exists anywhere else)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from recalgorithm_amd import _abi, _lib  # noqa: E402

header = (sys.argv[1:] + ["recalgo.h"])[0]
headers = _lib.every_header()
if header not in headers or len(sys.argv) > 2:
    sys.exit(f"usage: abi_record.py [{' | '.join(headers)}]")
version, path = headers[header].version, _abi.record_path(header)
lines = [ln for ln in open(path).read().splitlines() if ln.strip()] if os.path.exists(path) else []
lines = [ln for ln in lines if ln.startswith("#") or int(ln.split()[0]) != version]
lines.append(f"{version} {_abi.declaration_hash(header)}")
open(path, "w").write("\n".join(lines) + "\n")
print(lines[-1])
