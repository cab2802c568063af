"""What tests/test_mlp_host.py and tests/test_gpu_mlp_kernels.py share: the shape lists of the GPU cases and the input
generator, so that the CPU module checks the bounds of tests/mlp_ref.py at the very shapes and numbers the GPU module
runs.  Fixtures only: the references live in tests/mlp_ref.py, what each shape reaches is asserted in the GPU module."""
import torch

F64 = torch.float64

HIDDEN = ((1,), (32,), (32, 1), (1, 1, 1), (32, 32, 32), (7, 32, 5), (24, 32, 7))
ACTS = ("relu", "leaky_relu", "identity")
# (FD, Dn): the input widths of the GPU module's fwd / bwd cases (what each reaches is asserted there, from the source)
LOADER_SHAPES = ((0, 1), (0, 37), (0, 448), (4, 0), (64, 0), (128, 0), (60, 4), (64, 1), (96, 0), (112, 3), (432, 16),
                 (192, 40), (256, 33), (320, 64), (416, 13), (416, 32), (448, 0), (128, 5))
BIG_BATCHES, SMALL_BATCHES = (255, 256, 257), (1, 31, 32)


def loader_cases():
    """(FD, Dn, B, hidden, act): every loader shape at B = 33, at one batch >= 255 and at one batch <= 32, the hidden
    widths and activations spread over them (3 and 7 are coprime: every width list meets every kind of batch)."""
    out = []
    for i, (FD, Dn) in enumerate(LOADER_SHAPES):
        for j, B in enumerate((33, BIG_BATCHES[i % 3], SMALL_BATCHES[(i // 3) % 3])):
            out.append((FD, Dn, B, HIDDEN[(3 * i + j) % 7], ACTS[(i + j) % 3]))
    return out


GRID_STRIDE_CASES = ((64, 3, 2 * 256 * 32 + 17, (32, 32), "relu"), (8, 0, 65_536 + 33, (7, 32, 5), "leaky_relu"))


def make_mlp_inputs(FD, Dn, B, hidden, seed=0):
    """fp32 inputs of one case, on the CPU (the GPU module moves them over: both modules see the same numbers).
    W0 is scaled by 1 / sqrt(K) so that the hidden values stay O(1) at every width."""
    gen = torch.Generator().manual_seed(1000 * seed + 7 * FD + 3 * Dn + B + 11 * len(hidden) + hidden[0])
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float32)
    dims = [FD + Dn] + list(hidden)
    return dict(
        xe=rn(B, FD), xd=rn(B, Dn) if Dn else None,
        Ws=[rn(dims[l], dims[l + 1]) * (dims[l] ** -0.5) for l in range(len(hidden))],
        bs=[rn(dims[l + 1]) * 0.1 for l in range(len(hidden))],
        w_out=rn(hidden[-1]) * 0.5, w0=rn(1) * 0.3, g=rn(B) * 0.5)


def fm_sum32(xe, D):
    """front_refs.embed_fwd_ref's definition S = sum_f E in float64, rounded once to fp32: [B, D]."""
    B, FD = xe.shape
    return xe.to(F64).reshape(B, FD // D, D).sum(1).to(torch.float32)
