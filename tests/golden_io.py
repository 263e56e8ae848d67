"""Reading the learn-step fixtures of tests/golden/.

No committed file is larger than 1 MiB, so make_golden.py (save_fixture) stores a fixture that would be
larger in two files: `<name>.npz` with everything but the Adam moments, and `<name>.npz.part2` (also an
npz archive) with the `m_<i>` / `v_<i>` arrays.  load_fixture gives both as one mapping."""
import os

import numpy as np


def load_fixture(path):
    z = dict(np.load(path))
    if os.path.exists(path + ".part2"):
        more = np.load(path + ".part2")
        assert not set(more.files) & set(z), path
        z.update(more)
    return z
