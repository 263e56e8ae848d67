"""`.pack` checkpoint interop with the reference's own Network.save / Network.load, bit for bit
(VERDICT r4 missing #2), from stored fixtures.

tests/golden/ref_<case>.pack are checkpoints the REFERENCE's Network.save wrote (large ones in parts);
tests/golden/pack_interop.json records their metadata and the shape and sha256 of every tensor the
reference held when it saved.  `pack_interop.py golden` made them, after the reference loaded the
drop-in's checkpoints bit for bit.  Two directions:
  * reference -> drop-in: Network.load of the reference's file gives its metadata and every tensor
    bit for bit;
  * drop-in -> reference: Network.save of that network writes the reference's file byte for byte,
    so the reference's loader reads the drop-in's checkpoint exactly as it reads its own."""
import hashlib
import json
import os

import numpy as np
import torch

from dqn import Networks
from refnets import Box, hybrid_network_config, mlp_network_config

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
META_SAVED = (12345, 67, np.float64(3.5), 88.0)   # what the reference's save was called with


def test_pack_interop_both_directions(tmp_path):
    with open(os.path.join(GOLDEN, "pack_interop.json")) as f:
        rec = json.load(f)
    assert len(rec["cases"]) == 3
    for i, c in enumerate(rec["cases"]):
        case = c["case"]
        blob = b"".join(open(os.path.join(GOLDEN, name), "rb").read() for name in c["files"])
        assert hashlib.sha256(blob).hexdigest() == c["sha256"], case
        ref_pack = tmp_path / f"ref_{case}.pack"
        ref_pack.write_bytes(blob)
        cls = Networks.DuelingDeepQNetwork if c["head"] == "dueling" else Networks.DeepQNetwork
        conf = mlp_network_config if c["kind"] == "mlp" else hybrid_network_config
        torch.manual_seed(100 + i)
        net = cls(torch.device("cpu"), 1e-4, conf, Box(c["obs_dim"]), 8)
        # reference -> drop-in
        meta = net.load(str(ref_pack))
        assert tuple(meta) == tuple(rec["meta"]) == META_SAVED, (case, meta)
        got = {k: v.detach().cpu().numpy() for k, v in net.state_dict().items()}
        assert sorted(got) == sorted(c["tensors"]), (case, sorted(got))
        for k, want in c["tensors"].items():
            assert got[k].dtype == np.float32 and list(got[k].shape) == want["shape"], (case, k)
            assert hashlib.sha256(np.ascontiguousarray(got[k]).tobytes()).hexdigest() == want["sha256"], (case, k)
        # drop-in -> reference
        ours_pack = tmp_path / f"ours_{case}.pack"
        net.save(str(ours_pack), *META_SAVED)
        assert ours_pack.read_bytes() == blob, case
