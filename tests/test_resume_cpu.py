"""Resume, the parts that need no GPU: the halving ranking (a pure function), the refused engine_halving combinations (raised before
a loader is read or a population created), and the ctypes prototypes of the new C-ABI symbols."""
import ctypes
from types import SimpleNamespace

import pytest

NEW_SYMBOLS = ("mfas_population_train_from", "mfas_population_set_state", "mfas_population_get_progress",
               "mfas_population_set_progress", "mfas_population_move")


def test_halving_survivors_ranking():
    from mfas_amd.population import halving_survivors
    # the best ceil(K / eta), in input order
    assert halving_survivors([0.1, 0.5, 0.3, 0.4], [0, 0, 0, 0], 2) == [1, 3]
    assert halving_survivors([0.2], [0], 2) == [0]
    # ties go to the lower input index
    assert halving_survivors([0.5, 0.5, 0.5, 0.5], [0, 0, 0, 0], 2) == [0, 1]
    assert halving_survivors([0.1, 0.4, 0.4, 0.4, 0.2], [0] * 5, 2) == [1, 2, 3]
    assert halving_survivors([0.3, 0.4, 0.4], [0] * 3, 3) == [1]
    # a non-finite status ranks behind every finite candidate, whatever its metric; so does a metric that is no number
    assert halving_survivors([0.9, 0.1, 0.2, 0.0], [1, 0, 0, 0], 2) == [1, 2]
    assert halving_survivors([float("nan"), 0.0, float("inf"), 0.1], [0, 0, 0, 0], 2) == [1, 3]
    assert halving_survivors([0.9, 0.8, 0.1], [1, 1, 0], 2) == [0, 2]          # ... and among themselves by index
    assert halving_survivors([0.9, 0.8, 0.7], [1, 1, 1], 3) == [0]
    # eta = 3 with K = 7: ceil(7 / 3) = 3 survivors
    assert halving_survivors([0.1, 0.7, 0.3, 0.6, 0.2, 0.65, 0.0], [0] * 7, 3) == [1, 3, 5]
    assert halving_survivors([0.1, 0.7, 0.3, 0.6, 0.2, 0.65, 0.0], [0, 0, 0, 1, 0, 0, 0], 3) == [1, 2, 5]
    with pytest.raises(ValueError):
        halving_survivors([0.1, 0.2], [0, 0], 1)
    with pytest.raises(ValueError):
        halving_survivors([0.1, 0.2], [0], 2)


class _Untouchable:
    """Stands where a loader would: any use of it means something was read before the refusal."""

    def __getattr__(self, name):
        raise AssertionError(f"the refused call touched its dataloaders ({name})")

    def __iter__(self):
        raise AssertionError("the refused call iterated its dataloaders")


def _args(**kw):
    base = dict(vid_len=(8, 32), num_outputs=10, drpt=0.5, inner_representation_size=16, batchnorm=True, alphas=False, multitask=False,
                weightsharing=False, batchsize=20, eta_max=1e-3, eta_min=1e-6, Ti=1, Tm=2, use_dataparallel=False, verbose=False,
                epochs=10, engine_halving=(2, (1, 3)))
    base.update(kw)
    return SimpleNamespace(**base)


def test_refused_halving_combinations_raise_before_anything_is_created(monkeypatch):
    import mfas_amd as M
    from mfas_amd import engine, ntu_searchable as NS, population

    def no_population(*a, **kw):
        raise AssertionError("a population was created before the refusal")

    monkeypatch.setattr(engine.Population, "__init__", no_population)
    loaders = {"train": _Untouchable(), "dev": _Untouchable()}
    confs = [[[0, 0, 0]], [[1, 1, 1]]]
    cls = M.Searchable_Skeleton_Image_Net
    with pytest.raises(NotImplementedError, match="weightsharing"):
        M.train_sampled_models(confs, cls, loaders, _args(weightsharing=True), "cuda:0")
    with pytest.raises(NotImplementedError, match="return_model"):
        M.train_sampled_models(confs, cls, loaders, _args(), "cuda:0", return_model=[0])
    monkeypatch.setattr(population, "dist_info", lambda: (0, 2))
    with pytest.raises(NotImplementedError, match="world > 1"):
        M.train_sampled_models(confs, cls, loaders, _args(), "cuda:0")
    monkeypatch.setattr(population, "dist_info", lambda: (0, 1))
    for bad in ((1, (1,)), (2, ()), (2, (3, 1)), (2, (0, 2)), (2, (1, 10))):
        with pytest.raises(ValueError, match="engine_halving"):
            M.train_sampled_models(confs, cls, loaders, _args(engine_halving=bad), "cuda:0")
    assert NS._check_halving(_args(engine_halving=None), []) is None
    assert NS._check_halving(_args(), []) == (2, (1, 3))


def test_new_symbols_have_ctypes_prototypes():
    import __graft_entry__ as ge
    ge.build()
    from mfas_amd import _lib
    L = _lib.lib()
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTS, name
        fn = getattr(L, name)
        assert fn.argtypes is not None, f"{name}: no argtypes"
    P = ctypes.c_void_p
    assert list(L.mfas_population_train_from.argtypes) == [P, ctypes.POINTER(_lib.mfas_table), ctypes.POINTER(_lib.mfas_table), P, P,
                                                            ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, P, P]
    assert list(L.mfas_population_set_state.argtypes) == [P, ctypes.c_int32, ctypes.c_int32, P]
    assert list(L.mfas_population_get_progress.argtypes) == [P, ctypes.c_int32, P, P, P, P]
    assert list(L.mfas_population_set_progress.argtypes) == [P, ctypes.c_int32, P, P, P, P]
    assert list(L.mfas_population_move.argtypes) == [P, ctypes.c_int32, P, ctypes.c_int32]


def test_cli_flag_becomes_eta_and_rungs():
    import main_searchable_ntu as main
    assert main.parse_args([]).engine_halving is None
    assert main.parse_args(["--engine_halving", "2", "1", "3"]).engine_halving == (2, (1, 3))
    with pytest.raises(SystemExit):
        main.parse_args(["--engine_halving", "2"])
