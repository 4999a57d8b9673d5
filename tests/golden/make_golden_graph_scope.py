#!/usr/bin/env python3
"""Generate tests/golden/mol8_graph_scope.npz: the per-molecule reconstruction loss of the batched ``mol8`` case by
the reference's OWN model file (GAE.reconstruction_loss(g, scope="graph")).

For each of the 8 molecules of ``mol8_parts.npz``, with the ``mol8`` state dict, the reference's ``gae.py`` (imported
through ``make_golden.load_reference()`` and its DGL stand-in, neither edited) runs on that molecule ALONE; the loss of
train_inductive.py:44-48 is taken with that molecule's own label and pos_weight; the 8 losses are averaged and
backpropagated.  Two settings, as in make_golden.py: dropout 0 (``*_p0``) and the injected ``mol8`` mask rows of the
molecule (``*_p01``: the reference's decoder at dropout 0 applied to ``encode(g) * mask``, i.e. ``F.dropout``'s
multiplier given instead of drawn).

Only DATA is written.  Usage:  python tests/golden/make_golden_graph_scope.py"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402  (the reference loader and its DGL stand-in)


def per_molecule_loss(ref, whole, parts, masks):
    """(mean loss, [8] per-molecule losses, {param: grad}) of the reference model on each molecule alone"""
    hidden = [int(h) for h in whole["hidden"]]
    model = ref.GAE(whole["X"].shape[1], hidden)
    model.load_state_dict({k[3:]: torch.from_numpy(v) for k, v in whole.items() if k.startswith("sd/")})
    model.decoder.dropout = 0.0
    losses = []
    for i in range(int(parts["n_graphs"])):
        n = int(parts[f"g{i}/n"])
        g = make_golden.StubGraph(n, parts[f"g{i}/src"], parts[f"g{i}/dst"])
        g.ndata["h"] = torch.from_numpy(parts[f"g{i}/X"]).clone()
        if masks is None:
            logits = model(g)                                            # gae.py:47-53
        else:
            logits = model.decoder(model.encode(g) * torch.from_numpy(masks[i]))   # gae.py:70-71 with the given mask
        adj = g.adjacency_matrix().to_dense()                            # train_inductive.py:44
        pw = (adj.shape[0] * adj.shape[0] - adj.sum()) / adj.sum()       # :46
        losses.append(F.binary_cross_entropy_with_logits(logits, adj, pos_weight=pw))   # :48
    loss = torch.stack(losses).mean()
    model.zero_grad()
    loss.backward()
    grads = {k: p.grad.detach().numpy().copy() for k, p in model.named_parameters()}
    return loss.detach().numpy(), torch.stack(losses).detach().numpy(), grads


def main():
    torch.set_num_threads(1)          # bit-reproducible fp32 reductions (make_golden.py, "Reproducibility")
    ref = make_golden.load_reference()
    whole = dict(np.load(os.path.join(HERE, "mol8.npz")))
    parts = dict(np.load(os.path.join(HERE, "mol8_parts.npz")))
    offs = np.cumsum([0] + [int(parts[f"g{i}/n"]) for i in range(int(parts["n_graphs"]))])
    masks = [whole["mask"][offs[i]:offs[i + 1]] for i in range(len(offs) - 1)]
    out = {"node_ptr": offs.astype(np.int64)}
    for tag, m in (("p0", None), ("p01", masks)):
        loss, per, grads = per_molecule_loss(ref, whole, parts, m)
        out["loss_" + tag] = loss
        out["graph_loss_" + tag] = per
        for k, v in grads.items():
            out[f"grad_{tag}/{k}"] = v
    np.savez_compressed(os.path.join(HERE, "mol8_graph_scope.npz"), **out)
    print("wrote mol8_graph_scope", {k: np.shape(v) for k, v in out.items()})


if __name__ == "__main__":
    main()
