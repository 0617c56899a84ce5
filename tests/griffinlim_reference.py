"""The float64 restatement that pins Griffin-Lim: the definition on ``torch.stft`` / ``torch.istft`` / ``numpy.linalg.pinv``,
independent of the package's tables.  ``dtype=torch.float32`` runs the same composition in complex64 (the "CPU float32 composition" the
three-iteration test measures the kernels against).

    X_0 = S * P0;  C_-1 = 0;  beta = momentum / (1 + momentum);  tiny = 2^-126
    n_iter times:  x = ISTFT(X);  C = STFT(x);  A = C - beta * C_prev;  X = S * A / (|A| + tiny)
    y = ISTFT(X)
"""
import numpy as np
import torch

TINY = 2.0 ** -126


def hann_padded(win_length, n_fft, dtype=torch.float64):
    """The periodic Hann window of win_length centred in zeros (written out here, not taken from the package)."""
    w = torch.zeros(n_fft, dtype=torch.float64)
    left = (n_fft - win_length) // 2
    n = torch.arange(win_length, dtype=torch.float64)
    w[left:left + win_length] = 0.5 - 0.5 * torch.cos(2.0 * torch.pi * n / win_length)
    return w.to(dtype)


def signal(n, seed):
    """x[n] = 0.3 sin(2 pi 0.031 n + 3 sin(2 pi 0.0007 n)) + 0.1 sin(2 pi 0.12 n) + 0.02 N(0, 1), float64"""
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(n, dtype=torch.float64)
    return (0.3 * torch.sin(2 * torch.pi * 0.031 * t + 3.0 * torch.sin(2 * torch.pi * 0.0007 * t)) + 0.1 * torch.sin(2 * torch.pi * 0.12 * t)
            + 0.02 * torch.randn(n, generator=g, dtype=torch.float64))


def stft(x, w, n_fft, hop):
    """(L,) -> complex (1 + L // hop, n_bins): centred frames, zero padding"""
    if x.numel() == 0:
        return torch.zeros(1, n_fft // 2 + 1, dtype=torch.complex128 if x.dtype == torch.float64 else torch.complex64)
    return torch.stft(x, n_fft, hop, n_fft, window=w.to(x.dtype), center=True, pad_mode="constant", return_complex=True).T


def istft(X, w, n_fft, hop):
    """complex (T, n_bins) -> ((T - 1) * hop,)"""
    T = X.shape[0]
    if T < 2:
        return torch.zeros(0, dtype=X.real.dtype)
    return torch.istft(X.T, n_fft, hop, n_fft, window=w.to(X.real.dtype), center=True, length=(T - 1) * hop)


def project(C, C_prev, S, beta):
    """-> X_next = S * A / (|A| + tiny), A = C - beta * C_prev"""
    A = C - beta * C_prev
    return S * A / (A.abs() + TINY)


def griffin_lim(S, w, n_fft, hop, P0, n_iter, momentum=0.99, dtype=torch.float64):
    """S (T, n_bins) >= 0, P0 unit complex (T, n_bins) -> y ((T - 1) * hop,) in ``dtype``"""
    cdt = torch.complex128 if dtype == torch.float64 else torch.complex64
    beta = momentum / (1.0 + momentum)
    S = S.to(dtype)
    X = S * P0.to(cdt)
    C_prev = torch.zeros_like(X)
    for _ in range(n_iter):
        C = stft(istft(X, w, n_fft, hop), w, n_fft, hop)
        X, C_prev = project(C, C_prev, S, beta), C
    return istft(X, w, n_fft, hop)


def spectral_convergence(y, S, w, n_fft, hop):
    """|| |STFT64(y)| - S || / ||S||, float64"""
    S = S.double()
    return float((stft(y.double(), w, n_fft, hop).abs() - S).norm() / S.norm())


def mel_to_linear(c, mean, scale, basis, base):
    """float64: max(1e-10, pinv(B) @ base ** (c * scale + mean)); basis (n_mels, n_bins); the pseudo-inverse rounded to f32 once."""
    pinv = np.linalg.pinv(np.asarray(basis, dtype=np.float64)).astype(np.float32).astype(np.float64)       # (n_bins, n_mels)
    mel = float(base) ** (np.asarray(c, np.float64) * np.asarray(scale, np.float64) + np.asarray(mean, np.float64))
    return np.maximum(1e-10, mel @ pinv.T)
