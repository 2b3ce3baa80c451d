"""float64 closed forms of the two kernels behind the native DeBERTa's embedding-side gradients (csrc/deberta.hip):

  * ``embed_bwd_params``: the backward of ``LayerNorm(source) * mask`` (``mmf_deberta_embed``) with respect to the source rows and
    the LayerNorm's gamma / beta, the source rows being ``table[clamp(ids)]`` or ``embeds`` (``mmf_deberta_embed_bwd_params``);
  * ``scatter_add``: ``dtable[clamp(ids[r])] += d_rows[r]`` over the unmasked rows (``mmf_embedding_scatter_add_f32``).

Each also returns the summed magnitudes of the terms behind every output element: what an f32 evaluation's rounding noise is
measured against.  tests/test_deberta_embed_grad_cpu.py pins both against float64 torch autograd."""
import torch


def clamp_ids(ids, vocab):
    """the forward's clamp: an id outside the table names its nearest row"""
    return ids.long().clamp(0, vocab - 1)


def embed_bwd_params(dy, gamma, eps, mask=None, ids=None, table=None, embeds=None):
    """dy (rows, d), gamma (d,), mask (rows,) or None, and ids (rows,) with table (vocab, d) or embeds (rows, d)
    -> (d_rows (rows, d), dgamma (d,), dbeta (d,)), (the magnitudes of d_rows', dgamma's and dbeta's terms), all float64"""
    assert (ids is None) != (embeds is None)
    src = (table.double()[clamp_ids(ids, table.shape[0])] if ids is not None else embeds.double())
    dy, gamma = dy.double(), gamma.double()
    m = torch.ones(src.shape[0], 1, dtype=torch.float64) if mask is None else mask.double().reshape(-1, 1)
    mean = src.mean(-1, keepdim=True)
    rstd = (((src - mean) ** 2).mean(-1, keepdim=True) + eps).rsqrt()
    xh = (src - mean) * rstd
    g = dy * m * gamma
    s1, s2 = g.mean(-1, keepdim=True), (g * xh).mean(-1, keepdim=True)
    d_rows = torch.where(m != 0, rstd * (g - s1 - xh * s2), torch.zeros_like(g))
    dgamma, dbeta = (dy * m * xh).sum(0), (dy * m).sum(0)
    a1, a2 = g.abs().mean(-1, keepdim=True), (g * xh).abs().mean(-1, keepdim=True)
    mags = (rstd * (g.abs() + a1 + xh.abs() * a2), (dy * m * xh).abs().sum(0), (dy * m).abs().sum(0))
    return (d_rows, dgamma, dbeta), mags


def scatter_add(ids, d_rows, vocab, mask=None, fill=None):
    """-> (dtable (vocab, d) float64 = fill + the scatter, the number of unmasked occurrences of every table row (vocab,), the
    summed magnitudes |fill| + sum |d_rows[r]| (vocab, d))"""
    d_rows = d_rows.double()
    d = d_rows.shape[1]
    out = torch.zeros(vocab, d, dtype=torch.float64) if fill is None else fill.double().clone()
    mag, count = out.abs(), torch.zeros(vocab, dtype=torch.long)
    rows = clamp_ids(ids, vocab)
    for r in range(d_rows.shape[0]):
        if mask is not None and float(mask[r]) == 0.0:
            continue
        out[rows[r]] += d_rows[r]
        mag[rows[r]] += d_rows[r].abs()
        count[rows[r]] += 1
    return out, count, mag
