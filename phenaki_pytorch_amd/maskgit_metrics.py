"""Validation metrics of the masked-token transformer on the MI355X kernels: `MaskGitMetrics`, the accumulator over held-out batches of
`Phenaki.evaluate` -- the counterpart of metrics.TokenizerMetrics on the transformer side.

The reference's PhenakiTrainer samples videos from its EMA model every `save_results_every` steps and saves image grids
(phenaki_trainer.py:449-); it computes no number.  What a MaskGIT-style model is judged by are the masked-token perplexity, top-1 / top-5 accuracy,
the rank of the true token, the entropy of the predictive distribution and how well the token critic spots wrong fills.  `Phenaki.evaluate`
produces the per-token values without the (rows, 65 536) logits (pk_vocab_eval, csrc/sampler.hip); the accumulator adds no host
synchronisation until `compute()`.

top-k is `rank < k` throughout, with rank = the number of OTHER tokens scored above the true one; it is not `pred == target` (a tie at the top
would make the two differ).
"""
import math

import torch

from .metrics import merge_states


class MaskGitMetrics:
    """running validation statistics of a Phenaki model (MaskGit + optional token critic) over held-out batches.

        mm = MaskGitMetrics(phenaki)
        for ids, emb in held_out: mm.update(video_codebook_ids=ids, text_embeds=emb, generator=gen)   # device-side sums only
        numbers = mm.compute()                                                                         # one synchronisation: Python numbers

    update() takes the keyword arguments of `Phenaki.evaluate`.  state (device tensors): float64 sums of the per-token nll and entropy, int64 counts
    of the masked tokens and of those with rank < 1, < 5 and < 10, the int64 sum of the ranks and the float64 sum of 1 / (rank + 1); with a critic
    the float64 sum of its binary cross entropy over all positions and int64 counts of correct signs, of positive labels and of positions.

    compute() first sums the state over the ranks of an initialised process group (metrics.merge_states), then derives tokens, loss (mean nll, nats),
    perplexity = exp(loss), top1 / top5 / top10, mean_rank, mrr, entropy and, with a critic, critic_bce, critic_accuracy, critic_positive_share.
    With a process group of more than one rank it is a COLLECTIVE: every rank of the group calls it and gets the same numbers; a rank that validates
    on its own while the others go on calls compute(merge=False)."""

    def __init__(self, phenaki):
        self.phenaki = phenaki
        self.state = None

    def reset(self):
        self.state = None

    @staticmethod
    def step_state(r):
        """the state increment of one `Phenaki.evaluate` result"""
        rank = r['rank'].long()
        step = dict(nll=r['nll'].double().sum(), entropy=r['entropy'].double().sum(),
                    tokens=torch.full((), rank.numel(), dtype=torch.long, device=rank.device), top1=(rank < 1).sum(), top5=(rank < 5).sum(), top10=(rank < 10).sum(), rank=rank.sum(),
                    rrank=(1. / (rank.double() + 1.)).sum())
        if 'critic_logits' in r:
            x, y = r['critic_logits'].double(), r['critic_labels']
            bce = torch.nn.functional.binary_cross_entropy_with_logits(x, y.double(), reduction='sum')
            step.update(critic_bce=bce, critic_correct=((x > 0) == y).sum(), critic_labels=y.sum(),
                        critic_positions=torch.full((), y.numel(), dtype=torch.long, device=y.device))
        return step

    @torch.no_grad()
    def update(self, *args, **kwargs):
        step = self.step_state(self.phenaki.evaluate(*args, **kwargs))
        if self.state is None:
            self.state = step
        else:
            for k in step:
                self.state[k] = self.state[k] + step[k]
        return self

    @torch.no_grad()
    def compute(self, group=None, merge=True):
        if self.state is None:
            raise RuntimeError('MaskGitMetrics.compute() before any update()')
        s = {k: v.clone() for k, v in self.state.items()}
        if merge:
            s = merge_states(s, group)
        tokens = s['tokens'].double()
        vals = [tokens, s['nll'] / tokens, s['top1'] / tokens, s['top5'] / tokens, s['top10'] / tokens, s['rank'] / tokens, s['rrank'] / tokens,
                s['entropy'] / tokens]
        with_critic = 'critic_bce' in s
        if with_critic:
            pos = s['critic_positions'].double()
            vals += [s['critic_bce'] / pos, s['critic_correct'] / pos, s['critic_labels'] / pos]
        packed = torch.stack([v.double() for v in vals]).tolist()                      # the one synchronisation
        tokens, loss, top1, top5, top10, mean_rank, mrr, entropy = packed[:8]
        out = dict(tokens=int(tokens), loss=loss, perplexity=math.exp(loss) if loss < 700. else float('inf'), top1=top1, top5=top5, top10=top10,
                   mean_rank=mean_rank, mrr=mrr, entropy=entropy)
        if with_critic:
            out.update(critic_bce=packed[8], critic_accuracy=packed[9], critic_positive_share=packed[10])
        return out
