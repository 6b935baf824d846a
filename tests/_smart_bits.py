"""The recorded bits of the single-threshold lane-group SMART call
(tests/golden/smart_single_bits.json): the cases, and how one of them is run and digested.
tools/record_smart_bits.py writes the record with these functions and
tests/test_gpu_smart.py::test_single_threshold_bits_equal_the_record reads it with them.

In the butterfly layouts the C oracle carries no bits of that call (it sums in the reference's
order), and since the single-threshold call became the sweep kernel's one-column instance there
is no second closed-form kernel to compare with (with flags 0 there is the plain re-scan kernel,
tests/test_gpu_thresholds.py).  The record was taken from the last commit that still had one
(its hash is in the file): every layout of the sweep tests x both families x the three
flag pairs x the six distinct thresholds of TH7 and one per-sequence threshold vector.

Only DeviceBatch.pack and DeviceBatch.simulate_smart are used, always with a stats tensor, so
that flags (False, False) too run the lane-group kernel in the batch's own layout.
"""
import hashlib
import json
import os

import numpy as np

from tests import _thresholds_cases as C
from tests.test_gpu_thresholds import FLAG_PAIRS, LAYOUTS

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "smart_single_bits.json")
B, T = C.B, C.T
FAMILIES = C.FAMILIES


def thresholds():
    """{key: scalar or [B] thresholds}: TH7's distinct values in order, then the vector."""
    th = {float(t).hex(): t for t in dict.fromkeys(C.TH7)}
    assert len(th) == 6
    th["per_sequence"] = np.random.default_rng(12).uniform(-1.0, 30.0, B)
    return th


def case_id(P, d, name):
    return f"{P},{d},{name}"


def flag_id(pf, cc):
    return f"prefix={int(pf)},comparator={int(cc)}"


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def inputs_digest(f):
    """SHA-256 of the host arrays handed to pack: z [B, T, d] then y [B, T], float64."""
    return sha(np.asarray(f.z, dtype=np.float64), np.asarray(f.y, dtype=np.float64))


def run(eng, P, d, name):
    """One (layout, family): {"inputs", "layout", "runs": {flag pair: {threshold:
    [sha256 of regret[:B], sha256 of switch_step, re-scanned steps, closed comparators]}}}."""
    import torch
    f = C.family(name, d)
    db = eng.DeviceBatch(B, T, d, lanes_per_seq=P).pack(f.z, f.y)
    runs = {}
    for pf, cc in FLAG_PAIRS:
        cols = runs[flag_id(pf, cc)] = {}
        for key, th in thresholds().items():
            sw = torch.full((B,), -7, dtype=torch.int64, device=db.device)
            st = torch.zeros(2, dtype=torch.int64, device=db.device)
            reg = db.simulate_smart(th, C.SQ2, switch_step=sw, closed_prefix=pf,
                                    closed_comparator=cc, stats=st)
            torch.cuda.synchronize()
            stv = st.cpu().numpy()
            cols[key] = [sha(reg[:B].cpu().numpy()), sha(sw.cpu().numpy()),
                         int(stv[0]), int(stv[1])]
    return {"inputs": inputs_digest(f), "layout": [int(db.L.P), int(db.L.C), int(db.L.chain)],
            "runs": runs}


def load():
    with open(PATH) as fh:
        return json.load(fh)
