"""Child of tests/test_gpu_train_deterministic.py::test_bits_across_processes: a fresh process runs three deterministic training steps
of one sampled and one chunked-CSR case and prints a SHA-1 over the losses, the variables and the optimizer slots."""
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import numpy as np
    from tests.test_gpu_train_deterministic import _batch, _md, _model
    from coper_amd import data as cdata
    sha = hashlib.sha1()
    for name, route, chunk in (("cpg_mlp_bn", "sampled", 0), ("cpg_linear", "csr", 128)):
        md = _md(name)
        m = _model(md, cdata.synthetic_params(md, seed=21, ent_std=0.1), True, chunk)
        for step in range(3):
            loss = m.train_step(_batch(md, route, 77, 37, seed=700 + step)).cpu().numpy()
            sha.update(loss.tobytes())
        for k in sorted(m._tensors):
            sha.update(k.encode())
            sha.update(m._tensors[k].cpu().numpy().tobytes())
        slots, powers = m.optimizer_state()
        for k in sorted(slots):
            for part in slots[k]:
                sha.update(np.ascontiguousarray(part).tobytes())
        sha.update(repr(sorted(powers.items())).encode())
        m.close()
    print("DIGEST " + sha.hexdigest())


if __name__ == "__main__":
    main()
