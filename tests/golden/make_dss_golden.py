#!/usr/bin/env python3
"""Golden for tests/test_host_dss_vs_reference_binary.py: the seeded synthetic .bca of that test goes through
oracle/_ref/ref_harness (DSS::GetProfile / GetMuLetters of the unmodified reference objects, built by oracle/Makefile.ref);
per chain the md5 of its profile bytes and Mu letters, plus the md5 of the input file.  CPU only, a few seconds.
Output: tests/golden/dss_synthetic1500.json."""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import test_host_dss_vs_reference_binary as t  # noqa: E402


def main():
    with tempfile.TemporaryDirectory() as td:
        bca = t.write_input(td)
        chains = t.run_harness(td, bca)
        out = {"n": t.N, "seed": t.SEED, "bca_md5": t.file_md5(bca),
               "command": "ref_harness dbq syn.bca ref.rskdb -- -fast",
               "chains": [t.chain_digest(c.prof, c.mu) for c in chains]}
    with open(os.path.join(HERE, "dss_synthetic1500.json"), "w") as f:
        json.dump(out, f, indent=0)
        f.write("\n")


if __name__ == "__main__":
    main()
