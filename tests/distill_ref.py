"""Float64 restatement of the knowledge-distillation loss (reference models/multimodal_model.py:250-256) and of its
gradient with respect to the student logits, written out term by term so the kernel tests have something independent of
both the HIP code and torch's kl_div to hold the kernels to:

    loss      = T^2 * (1 / B) sum_b sum_c p_bc (log p_bc - log q_bc),   p = softmax(t / T),  q = softmax(s / T)
    d loss/ds = (T / B) (q - p)

A teacher probability that underflows to 0 contributes 0 (torch's xlogy)."""
import torch

F64 = torch.float64


def _log_softmax(x: torch.Tensor, T: float) -> torch.Tensor:
    z = (x - x.max(dim=1, keepdim=True).values) / T
    return z - torch.log(torch.exp(z).sum(dim=1, keepdim=True))


def kd_value_grad(student: torch.Tensor, teacher: torch.Tensor, T: float):
    """-> (loss: 0-d float64, dstudent: (B, C) float64)"""
    s, t = student.detach().to(F64).cpu(), teacher.detach().to(F64).cpu()
    B = s.shape[0]
    lq, lp = _log_softmax(s, T), _log_softmax(t, T)
    p, q = torch.exp(lp), torch.exp(lq)
    terms = torch.where(p > 0, p * (lp - lq), torch.zeros_like(p))
    loss = T * T * terms.sum() / B
    return loss, (T / B) * (q - p)


def kd_row_bound(student: torch.Tensor, teacher: torch.Tensor, T: float) -> float:
    """f32 error model of one row's T^2 * KL in the kernel (csrc/loss.hip), u = 2^-24, R = the widest row range:
    scaled differences z = (x - max) / T to 2u|z|; exp / log to 1 ulp; C-term sums to C u of their magnitude; the
    probabilities to (C + 4) u relative (the sum Z) and u |z| absolute (the exponent's argument).  Worst case, not typical."""
    u = 2.0 ** -24
    C = student.shape[1]
    R = max(float((x.max(dim=1).values - x.min(dim=1).values).max()) for x in (student.double(), teacher.double()))
    r = R / T
    kl = (4 + 2 * C) * r + 2 * r * min(r, C) + 2 * C + 8
    return u * T * T * kl


def kd_loss_bound(student: torch.Tensor, teacher: torch.Tensor, T: float, ref: float, weight: float = 1.0) -> float:
    """row bound (the mean of B rows) + the f32 batch sum, (B / 256 + 10) u of the value"""
    u = 2.0 ** -24
    B = student.shape[0]
    return weight * kd_row_bound(student, teacher, T) + (B / 256 + 10) * u * abs(ref)


def kd_grad_bound(student: torch.Tensor, T: float, weight: float = 1.0) -> float:
    """elementwise: weight (T / B) times q - p to (2 C + 8) u absolute, plus the final product's rounding"""
    u = 2.0 ** -24
    B, C = student.shape
    return weight * (T / B) * (2 * C + 10) * u
