"""Mirror of /root/reference/models/search/train_searchable/ntu.py for the HIP engine.

``train_ntu_track_acc`` (ntu.py:14-89) and ``test_ntu_track_acc`` (ntu.py:92-125) keep the reference
signatures; the epoch x {train, dev} x batch loop, CE loss, Adam step and best-dev tracking all run
inside the engine for a population of one.
"""
from __future__ import annotations

import torch

from .driver import _require_loader, etas_for, print_epoch_stats, tap_bits_of, train_one
from .engine import F1_FIXED_POINT, Population, best_dev_accuracy


def _adam_hyper(hp, optimizer):      # (train_mmimdb_track_f1 reads weight_decay ALONE from its optimizer: kept apart on purpose)
    if optimizer is not None and getattr(optimizer, "param_groups", None):
        g = optimizer.param_groups[0]
        hp.wd = float(g.get("weight_decay", hp.wd))
        hp.beta1, hp.beta2 = (float(b) for b in g.get("betas", (hp.beta1, hp.beta2)))
        hp.adam_eps = float(g.get("eps", hp.adam_eps))
    return hp


def train_ntu_track_acc(model, criteria, optimizer, scheduler, dataloaders, dataset_sizes,
                        device=None, num_epochs=200, verbose=False, multitask=False):
    """Trains ``model.central_params()`` with Adam (hyper-parameters read from ``optimizer``; the engine
    starts from a fresh Adam state like a newly built torch.optim.Adam) under the per-batch LR of
    ``scheduler``; returns the best dev accuracy (0-d float64 tensor) and leaves the best-epoch weights in
    ``model`` in eval mode (ntu.py:82-87).  ``criteria`` is CrossEntropyLoss by construction of the path."""
    train_l = _require_loader(dataloaders["train"], "train", device)
    dev_l = _require_loader(dataloaders["dev"], "dev", device)
    device = torch.device(device) if device is not None else train_l.table.device
    model = model.module if isinstance(model, torch.nn.DataParallel) else model
    hp = _adam_hyper(model.hyper(multitask), optimizer)
    hp.B = train_l.batch_size
    hp.tap_bits = tap_bits_of(train_l.table, dev_l.table)
    N_tr, N_dev = len(train_l.table), len(dev_l.table)
    etas = etas_for(scheduler, optimizer, num_epochs, -(-N_tr // hp.B))
    seed = int(torch.randint(0, 2 ** 31 - 1, (1,)).item())
    stats, _ = train_one(model, hp, train_l, dev_l, num_epochs, etas, device, drop_seed=seed, order_seed=seed + 1)
    if verbose:
        print_epoch_stats(stats[0], N_tr, N_dev)
    return torch.tensor(best_dev_accuracy(stats[0], N_dev), dtype=torch.float64)


def test_ntu_track_acc(model, dataloaders, dataset_sizes, device=None, multitask=False):
    """Accuracy over dataloaders['test'] in eval mode (ntu.py:92-125)."""
    test_l = _require_loader(dataloaders["test"], "test", device)
    device = torch.device(device) if device is not None else test_l.table.device
    model = model.module if isinstance(model, torch.nn.DataParallel) else model
    model.train(False)
    # (tap_bits stays unset here: setting it can change the plan, and with it the summation order)
    pop = Population(model.hyper(multitask), [model.conf], device)
    pop.set_params(0, model.flat_params())
    _, corr = pop.forward(0, test_l.table, count=True)
    pop.close()
    return torch.tensor(corr / float(len(test_l.table)), dtype=torch.float64)


def format_report(rep, names, n):
    """The lines --report prints for Population.evaluate(report=True)'s "report": per slot (`names`: the members, then the ensemble)
    top-1 / top-5 and the five worst classes (single-label), or the micro / macro / weighted F1 (multi-label)."""
    lines = []
    for s, name in enumerate(names):
        if "label_counts" in rep:
            lines.append("{} F1 micro: {:.4f} macro: {:.4f} weighted: {:.4f}".format(name, rep["f1_micro"][s], rep["f1_macro"][s],
                                                                                 rep["f1_weighted"][s]))
        else:
            acc = rep["per_class_accuracy"][s]
            worst = sorted((c for c in range(len(acc)) if acc[c] == acc[c]), key=lambda c: (acc[c], c))[:5]
            lines.append("{} top-1: {:.4f} top-5: {:.4f} worst classes: {}".format(
                name, rep["topk"][1][s] / n, rep["topk"][5][s] / n, ", ".join("{} ({:.3f})".format(c, acc[c]) for c in worst)))
    return lines


def test_population_track_acc(pop, dataloaders, dataset_sizes, members=None, weights=None, report=False):
    """The population form of test_ntu_track_acc (ntu.py:92-125): the accuracy of every member of `pop` (a Population) over
    dataloaders['test'] in eval mode, and that of their weighted ensemble (mean of the members' probabilities), from ONE
    Population.evaluate call.  Returns (float64 tensor [M] of member accuracies, 0-d float64 tensor: the ensemble's).  With
    loss_mode 1 both are F1 'samples' averages.  report=True (--report) also prints, per member and for the ensemble, top-1 / top-5
    and the five worst classes, or the micro / macro / weighted F1 (format_report), from the same call."""
    test_l = _require_loader(dataloaders["test"], "test", pop.device)
    n = float(len(test_l.table))
    res = pop.evaluate(test_l.table, members=members, weights=weights, report=report)
    if report:
        idx = range(pop.K) if members is None else members
        for line in format_report(res["report"], ["Member {} (candidate {})".format(s, int(k)) for s, k in enumerate(idx)] + ["Ensemble"], n):
            print(line)
    scale = 1.0 / F1_FIXED_POINT if pop.hp.loss_mode == 1 else 1.0
    member = torch.tensor([float(c) * scale / n for c in res["member_stats"]["dev_corrects"]], dtype=torch.float64)
    return member, torch.tensor(float(res["ensemble"]["corrects"]) * scale / n, dtype=torch.float64)
