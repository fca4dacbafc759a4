"""python tests/resume_entry_driver.py <dir> app:<yml> [--key value ...]: train.py's entry point with a checkpoint writer that, besides
what it always writes, keeps a copy of every epoch's checkpoint as <dir>/epoch<k>/latest_checkpoint.pt (tests/test_resume_entry_gpu.py
resumes a second run from one of them).  The copy is one more torch.save of the dict the run writes: nothing the run computes changes."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import train as T  # noqa: E402


def main():
    keep = sys.argv[1]
    sys.argv = [os.path.join(ROOT, "train.py")] + sys.argv[2:]
    write = T.checkpoint_state

    def keeping(*args, **kw):
        state = write(*args, **kw)
        d = os.path.join(keep, "epoch%d" % state["last_epoch"])
        os.makedirs(d, exist_ok=True)
        torch.save(state, os.path.join(d, "latest_checkpoint.pt"))
        return state

    T.checkpoint_state = keeping
    T.main()


if __name__ == "__main__":
    main()
