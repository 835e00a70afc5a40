"""What the tree GPU modules share (tests/test_tree_gpu.py, test_trees_gpu.py, test_tree_sweep_gpu.py, test_trees_sweep_gpu.py): the constants of their contracts,
the fixtures -- imported into each module, module-scoped there -- and the helpers that open contexts, make the 424 x 280 natural picture and ask the CPU oracle."""
import numpy as np
import pytest

SIZES = (128, 64, 32, 16)
W, H = 424, 280      # six 128 roots, no 64 roots, 8 roots at 32, 26 at 16; 576 nodes at most
LOGIT_TOL = 1e-3     # the logit contract (tests/test_hip_parity.py)
UNDECIDABLE = 4e-5   # tests/test_tree_gpu.py: a reference top-2 margin at or below it is a tie of the reference's own arithmetic
MLT_ERR_ARG, MLT_ERR_SIZE_DISABLED = 1, 4
TREE_ALL = ("leaf_map", "logits", "decisions", "candidates")
CHUNK = 4096         # the context's pass size


@pytest.fixture(scope="module")
def gpu(pkg):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    pkg.build.build_lib()
    return pkg


def blobs(pkg, seed, sizes=SIZES):
    return {s: pkg.weights.synthetic_blob(pkg.synth.ARCH_CTU if s == 128 else pkg.synth.ARCH_CU, seed) for s in sizes}


def open_context(pkg, seed, sizes=SIZES, **kw):
    return pkg.MltCnn(device=0, sizes=sizes, blobs=blobs(pkg, seed, sizes), head_index={s: 0 for s in sizes}, **kw)


@pytest.fixture(scope="module")
def contexts(gpu):
    """One context per (weight seed, sizes, flags), shared by the tests of the module (a test that sets a gate or a policy puts the default back)."""
    made = {}

    def get(seed, sizes=SIZES, flags=0):
        if (seed, sizes, flags) not in made:
            made[(seed, sizes, flags)] = open_context(gpu, seed, sizes, flags=flags)
        return made[(seed, sizes, flags)]
    yield get
    for m in made.values():
        m.close()


def natural_picture(pkg, pic_seed):
    """Twelve natural patches of 128 x 128 tiled 4 x 3 and cropped to 424 x 280 (org from the org patches, pred from the pred patches)."""
    org, pred = pkg.synth.natural_patches(128, 12, pic_seed)
    tile = lambda p: np.ascontiguousarray(p.reshape(3, 4, 128, 128).transpose(0, 2, 1, 3).reshape(384, 512)[:H, :W])
    return tile(org), tile(pred)


@pytest.fixture(scope="module")
def naturals(gpu):
    """naturals(seed) -> the natural picture of that seed, made once per module."""
    made = {}

    def get(seed):
        if seed not in made:
            made[seed] = natural_picture(gpu, seed)
        return made[seed]
    return get


def cut(pic, xy, S):
    return np.stack([pic[y:y + S, x:x + S] for x, y in xy])


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def reruns(m, sizes=SIZES):
    return sum(m.arithmetic(s)["guard_reruns"] for s in sizes)


def oracle_level(pkg, weight_seed, size, org, pred, xy, poc, qp):
    """The CPU oracle on the CUs at xy of one picture -> (split, top-2 margin of the decision head)."""
    import oracle
    net = oracle_level.nets.setdefault((weight_seed, size), oracle.Oracle(blobs(pkg, weight_seed, (size,))[size]))
    n = len(xy)
    logits, split = net.forward(cut(org, xy, size), cut(pred, xy, size), np.full(n, poc, np.int32), np.full(n, qp, np.int32), head_index=0)
    return split, pkg.decisions.from_logits(size, logits, head_index=0)["margin"]


oracle_level.nets = {}


class Pair:
    """An uploaded picture pair, closed on exit."""
    def __init__(self, m, org, pred):
        h, w = org.shape
        self.o, self.p = m.picture(w, h).upload(org), m.picture(w, h).upload(pred)

    def __enter__(self):
        return self.o, self.p

    def __exit__(self, *exc):
        self.o.close()
        self.p.close()
