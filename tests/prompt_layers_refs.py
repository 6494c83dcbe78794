"""Deep prompt tuning against the CPU oracle, without editing it: `deep_prompts` swaps wrappers in for
oracle.deberta_oracle.layer and .emd while it is open and puts the originals back on exit.

The oracle knows nothing of prompt rows.  What deep prompt tuning does to it is a change of the INPUT of encoder layer i
(1 <= i < D): the prompt slots T .. T+P-1 of every sample hold that layer's prompt tensor instead of what the layer below left
there.  The `layer` wrapper rebuilds `hidden` for exactly those calls -- encoder calls (query_states is None) of a layer index
in 1 .. D-1 -- by torch.cat of the video rows, the expanded prompt tensor and the text rows, so autograd of the oracle's scalar
gives the prompt tensors (leaves) their gradient and sends nothing from the slots into the layer below.  With D == nL the
enhanced mask decoder's key/value stream hs[-2] (and the hs[-2] inside q0 = pos_emb + hs[-2]) is the input of layer nL-1: the
`emd` wrapper rebuilds it the same way."""
import contextlib

import torch

from oracle import deberta_oracle as O


def overwrite(hidden, prompt, T):
    """hidden [B, S, H] with rows T .. T+P-1 of every sample replaced by prompt [P, H] (out of place: autograd sees a cat)"""
    B, P = hidden.shape[0], prompt.shape[0]
    return torch.cat([hidden[:, :T], prompt.to(hidden.dtype).expand(B, -1, -1), hidden[:, T + P:]], 1)


@contextlib.contextmanager
def deep_prompts(prompts, T, n_layers):
    """prompts: {layer index i: tensor [P, H]} for i = 1 .. D-1 (autograd leaves when their gradient is wanted)"""
    layer0, emd0 = O.layer, O.emd
    assert all(1 <= i < n_layers for i in prompts)

    def layer(hidden, mask4d, rel_pos, rel_emb, P, prefix, cfg, query_states=None):
        i = int(prefix.rsplit(".", 1)[1])
        if query_states is None and i in prompts:
            hidden = overwrite(hidden, prompts[i], T)
        return layer0(hidden, mask4d, rel_pos, rel_emb, P, prefix, cfg, query_states)

    def emd(hs, pos_emb, mask4d, rel_pos, rel_emb, P, cfg):
        if (n_layers - 1) in prompts:
            hs = list(hs)
            hs[-2] = overwrite(hs[-2], prompts[n_layers - 1], T)
        return emd0(hs, pos_emb, mask4d, rel_pos, rel_emb, P, cfg)

    O.layer, O.emd = layer, emd
    try:
        yield
    finally:
        O.layer, O.emd = layer0, emd0
