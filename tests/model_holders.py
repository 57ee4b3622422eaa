"""The ways a caller may go on holding a small round's model after dropping the list of arrays the
round returned (fedn_amd/smallround.py's result blocks must stay unwritten through each): shared by
tests/test_smallround_blocks.py (CPU) and tests/test_gpu_smallround.py."""
import numpy as np
import torch

# name -> what the caller keeps of ``model`` (a list of arrays; [1] is non-empty in every layout used)
HOLDERS = {
    "tensor": lambda model: torch.from_numpy(model[1]),
    "memoryview": lambda model: memoryview(model[1]),
    "frombuffer": lambda model: np.frombuffer(model[1], np.uint8),
    "array_slice": lambda model: model[1][3:7],
    "tensor_slice": lambda model: torch.from_numpy(model[1])[3:7],
}


def held_bytes(holder):
    """The bytes ``holder`` reaches, as a fresh uint8 array."""
    return np.asarray(holder).reshape(-1).view(np.uint8).copy()
