"""Host featurisation against the reference itself on chains no fixture has seen: 1500 synthetic CA traces go through
oracle/_ref/ref_harness (DSS::GetProfile / GetMuLetters of the unmodified reference objects) and through
rsk_dss_featurize; profiles and Mu letters must be byte-identical.  (This comparison, at 3000 chains, found the one
residue in ~500,000 where a double-precision GetDist flips a nearest-neighbour tie.)  CPU only.  The harness's output is
committed as per-chain digests (tests/golden/dss_synthetic1500.json, made by tests/golden/make_dss_golden.py), so the
comparison runs where the harness was not built; where it was, the harness is run as well."""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

import fixtures as fx
from reseek_amd import capi

ROOT = os.path.dirname(os.path.dirname(fx.GOLDEN))
HARNESS = os.path.join(ROOT, "oracle", "_ref", "ref_harness")
GOLDEN = os.path.join(fx.GOLDEN, "dss_synthetic1500.json")
N, SEED = 1500, 123


def write_input(td):
    """the seeded synthetic .bca of N chains (SCOP40 lengths) -> its path"""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bench
    import bench_search
    lens = bench.scop40_lengths()
    rng = np.random.default_rng(SEED)
    bca = os.path.join(td, "syn.bca")
    bench_search.write_bca(bca, lens[rng.choice(len(lens), N)], rng)
    return bca


def file_md5(path):
    with open(path, "rb") as f:
        return hashlib.md5(f.read()).hexdigest()


def chain_digest(prof, mu):
    """md5 of the feature-major profile bytes [8, L] and the Mu letters [L]"""
    h = hashlib.md5(np.ascontiguousarray(prof, np.uint8).tobytes())
    h.update(b"|")
    h.update(np.ascontiguousarray(mu, np.uint8).tobytes())
    return h.hexdigest()


def run_harness(td, bca):
    ref = os.path.join(td, "ref.rskdb")
    subprocess.run([HARNESS, "dbq", bca, ref, "--", "-fast"], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return fx.read_rskdb(ref)


def test_profiles_and_mu_letters_of_synthetic_chains():
    with open(GOLDEN) as f:
        golden = json.load(f)
    with tempfile.TemporaryDirectory() as td:
        bca = write_input(td)
        assert file_md5(bca) == golden["bca_md5"]          # the chains the committed digests were taken of
        chains = run_harness(td, bca) if os.path.exists(HARNESS) else None
        assert len(golden["chains"]) == N and (chains is None or len(chains) == N)
        nres = 0
        for i in range(N):
            _, seq, x, y, z = capi.bca_read_chain(bca, i)
            prof, mu = capi.dss_featurize(seq, x, y, z)
            assert chain_digest(prof, mu) == golden["chains"][i], (i, len(seq))
            if chains is not None:
                c = chains[i]
                assert np.array_equal(prof, c.prof) and np.array_equal(mu, c.mu), (i, len(seq))
            nres += len(seq)
        assert nres > 200000
