"""Conformer encoder/decoder stack on the HIP path (host-side schedule only).

Mirrors jatts.modules.conformer.encoder.Encoder.forward (encoder.py:233-289) and
EncoderLayer.forward (encoder_layer.py:78-178) for eval mode, normalize_before=True,
legacy relative positional attention, on PACKED RAGGED batches: every utterance is
processed exactly as the reference's B=1 ``inference()`` does (no pad leakage; SURVEY
§8 note N1).  All arithmetic is in libjatts_hip.so; this file only packs weights once
and sequences kernel launches.
"""
import math

import torch

from .. import hip
from ..hip import ACT_NONE, ACT_RELU

LN_EPS = 1e-12  # modules/transformer/layer_norm.py:23
BN_EPS = 1e-5   # torch.nn.BatchNorm1d default
PE_TABLE_LEN = 5000  # modules/positional_encoding.py:26


def legacy_rel_pos_table(n, d, table_len):
    """pe[p] = sin/cos((L-1-p) w_i), p < n  (positional_encoding.py:36-57, reverse=True).
    Built on the host in f32 exactly like the reference builds its buffer."""
    position = torch.arange(table_len - 1, -1, -1.0, dtype=torch.float32)[:n].unsqueeze(1)
    div_term = torch.exp(torch.arange(0, d, 2, dtype=torch.float32) * -(math.log(10000.0) / d))
    pe = torch.zeros(n, d, dtype=torch.float32)
    pe[:, 0::2] = torch.sin(position * div_term)
    pe[:, 1::2] = torch.cos(position * div_term)
    return pe


def rel_pos_table_new(cap, d):
    """RelPositionalEncoding (positional_encoding.py:265-309): row m encodes relative position
    cap-1-m, m in [0, 2cap-1); independent of the reference's table length."""
    pos = torch.arange(cap - 1, -cap, -1.0, dtype=torch.float32).unsqueeze(1)
    div_term = torch.exp(torch.arange(0, d, 2, dtype=torch.float32) * -(math.log(10000.0) / d))
    pe = torch.zeros(2 * cap - 1, d, dtype=torch.float32)
    pe[:, 0::2] = torch.sin(pos * div_term)
    pe[:, 1::2] = torch.cos(pos * div_term)
    return pe


class SpkProjection:
    """_integrate_with_spk_embed (models/fastspeech2.py:737-761; the same method in matchatts.py:560-584, matchatts_mas.py:644-668,
    vits.py:681-705).  "add": hs += projection(normalize(spembs)).  "concat": projection(cat[hs, normalize(spembs) broadcast over time])
    -- the Linear over the concatenation is split by columns, W [hs; s] = W_h hs + (W_s s + b): one k = 1 conv over the frames plus a
    per-utterance vector, so the (B, T, adim + D) concatenation never exists."""

    def __init__(self, sd, adim, kind, dtype, device):
        if kind not in ("add", "concat"):
            raise NotImplementedError("support only add or concat.")       # the reference's own message (:759)
        w, b = sd["projection.weight"], sd["projection.bias"]
        self.kind, self.A, self.dtype = kind, adim, dtype
        if kind == "add":
            self.h, self.s = None, hip.PackedConv(w, b, dtype, device)
        else:
            if w.shape[1] <= adim:
                raise ValueError("projection.weight: 'concat' expects (adim, adim + spk_embed_dim)")
            self.h, self.s = hip.PackedConv(w[:, :adim], None, dtype, device), hip.PackedConv(w[:, adim:], b, dtype, device)

    def __call__(self, rb, hs, spembs):
        """hs: f32 (rows, adim) of the ragged batch rb; spembs: (n_seq, D).  -> hs with the speaker integrated (in place for "add")."""
        dev, B = hs.device, rb.n_seq
        rbs = hip.RaggedBatch([1] * B, dev)
        sp = hip.l2_normalize(spembs.to(dev).float().reshape(B, -1).contiguous(), self.dtype, ldy=self.s.c_in)
        vec = self.s(rbs, sp, out_f32=True)
        if self.h is not None:
            hs = self.h(rb, hip.affine_cast(hs, self.dtype), out_f32=True)
        hip.add_seq_vector(rb, hs, vec)
        return hs


class ConformerRunner:
    def __init__(self, sd, prefix, n_heads, dtype, device, rel_style="legacy"):
        """rel_style: "legacy" = LegacyRelPositionalEncoding + LegacyRelPositionMultiHeadedAttention
        (FastSpeech2 / Matcha, fastspeech2.py fallback), "new" = RelPositionalEncoding +
        RelPositionMultiHeadedAttention (VITS text encoder and decoder)."""
        self.dtype, self.device, self.H = dtype, device, n_heads
        self.operand = hip.operand_code() if dtype == hip.F32 else dtype   # saved: the run-time packed position operands (_pos) follow the weights'
        self.split = self.operand == hip.F32S     # set_precision("fp32_split"): the attention takes the split arithmetic
        self.attn = hip._ATTENTION[0]     # set_precision(..., attention=): None = as the precision implies (hip.attention_dtype)
        self.rel_style = rel_style
        g = lambda k: sd[prefix + k]  # noqa: E731
        self.n_layers = 0
        while (prefix + f"encoders.{self.n_layers}.norm_mha.weight") in sd:
            self.n_layers += 1
        self.A = g("encoders.0.norm_mha.weight").shape[0]
        self.dk = self.A // n_heads
        if self.A % 64 or self.dk % 32:
            raise NotImplementedError("attention_dim must be a multiple of 64 and d_k a multiple of 32 (MFMA tiles)")
        f32 = lambda t: t.detach().float().to(device).contiguous()  # noqa: E731
        self.layers = []
        for i in range(self.n_layers):
            p = f"encoders.{i}."
            L = {}
            has = lambda k: (prefix + p + k) in sd  # noqa: E731
            for nm in ("norm_ff", "norm_mha", "norm_ff_macaron", "norm_conv", "norm_final"):
                if has(nm + ".weight"):
                    L[nm] = (f32(g(p + nm + ".weight")), f32(g(p + nm + ".bias")))
            for ff in ("feed_forward", "feed_forward_macaron"):
                if has(ff + ".w_1.weight"):
                    L[ff] = (hip.PackedConv(g(p + ff + ".w_1.weight"), g(p + ff + ".w_1.bias"), dtype, device),
                             hip.PackedConv(g(p + ff + ".w_2.weight"), g(p + ff + ".w_2.bias"), dtype, device))
            a = p + "self_attn."
            wq, wk = g(a + "linear_q.weight"), g(a + "linear_k.weight")
            if (2 * self.A) % 256 == 0:     # Q | K | V as ONE launch (jatts_conv_desc.n_split): Q | K row-major, V transposed
                L["qkv"] = hip.PackedConv(torch.cat([wq, wk, g(a + "linear_v.weight")], 0),
                                      torch.cat([g(a + "linear_q.bias"), g(a + "linear_k.bias"), g(a + "linear_v.bias")], 0), dtype, device)
            else:                           # Q | K and V as two launches
                L["qk"] = hip.PackedConv(torch.cat([wq, wk], 0), torch.cat([g(a + "linear_q.bias"), g(a + "linear_k.bias")], 0),
                                     dtype, device)
                L["v"] = hip.PackedConv(g(a + "linear_v.weight"), g(a + "linear_v.bias"), dtype, device)
            L["o"] = hip.PackedConv(g(a + "linear_out.weight"), g(a + "linear_out.bias"), dtype, device)
            L["rel"] = has("self_attn.linear_pos.weight")
            if L["rel"]:
                L["pos"] = hip.PackedConv(g(a + "linear_pos.weight"), None, dtype, device)
                L["u"] = f32(g(a + "pos_bias_u"))
                L["vb"] = f32(g(a + "pos_bias_v"))
            if has("conv_module.pointwise_conv1.weight"):
                c = p + "conv_module."
                L["pw1"] = hip.PackedConv(g(c + "pointwise_conv1.weight"), g(c + "pointwise_conv1.bias"), dtype, device)
                L["pw2"] = hip.PackedConv(g(c + "pointwise_conv2.weight"), g(c + "pointwise_conv2.bias"), dtype, device)
                wd = g(c + "depthwise_conv.weight").detach().float()
                L["dw_w"] = f32(wd.reshape(wd.shape[0], wd.shape[-1]))
                s = g(c + "norm.weight").detach().float() / torch.sqrt(g(c + "norm.running_var").detach().float() + BN_EPS)
                t = g(c + "norm.bias").detach().float() + (g(c + "depthwise_conv.bias").detach().float()
                                                            - g(c + "norm.running_mean").detach().float()) * s
                L["dw_s"], L["dw_t"], L["dw_k"] = f32(s), f32(t), wd.shape[-1]
            self.layers.append(L)
        self.after_norm = None
        if (prefix + "after_norm.weight") in sd:
            self.after_norm = (f32(g("after_norm.weight")), f32(g("after_norm.bias")))
        self.pe_len = PE_TABLE_LEN   # sticky, like the reference's regrown buffer (extend_pe)
        self._pos_cache = hip.DeviceCache("ConformerRunner._pos", max_entries=8)         # cap -> per-layer (per-head packed P, cv)

    def table_len(self, t_max):
        """Length of the positional table a run over t_max positions uses: the values of the legacy table depend on it, so it belongs to the
        signature of a captured graph (a graph captured before a regrowth holds the old tables)."""
        return max(self.pe_len, t_max)

    # -- positional projections: P_l = linear_pos_l(pe[:cap]); batch independent, cached per cap
    def _pos(self, t_max):
        if t_max > self.pe_len:  # positional_encoding.py:36-43: table regrown, values change
            self.pe_len = t_max
            self._pos_cache.clear()
        cap = hip.round_up(t_max, 128)
        return cap, self._pos_cache.get(cap, self.device, lambda: self._pos_build(cap))

    def _pos_build(self, cap):
        if self.rel_style == "new":
            pe = rel_pos_table_new(cap, self.A)          # (2cap-1, A)
        else:
            n_valid = min(cap, self.pe_len)
            pe = torch.zeros(cap, self.A, dtype=torch.float32)
            pe[:n_valid] = legacy_rel_pos_table(n_valid, self.A, self.pe_len)
        n_pos = pe.shape[0]
        pe_t = hip.affine_cast(pe.to(self.device), self.dtype)
        rb = hip.RaggedBatch([n_pos], self.device)
        per_layer = []
        for L in self.layers:
            if not L["rel"]:
                per_layer.append(None)
                continue
            P = L["pos"](rb, pe_t)                                                             # (cap, A)
            cv = hip.rowdot(P, self.A, n_pos, self.H, self.dk, L["vb"]).t().contiguous()      # (H, n_pos)
            # per-head weight operand of the BD GEMM (n = position m, contraction d_k): pure re-layout
            heads = [hip.operand(self.operand, P[:, h * self.dk:(h + 1) * self.dk].float().unsqueeze(-1)) for h in range(self.H)]
            per_layer.append((heads, cv))
        return per_layer

    def _ffn(self, rb, x, ln, ff, scale):
        xn = hip.layernorm(x, ln[0], ln[1], self.dtype, LN_EPS)
        w1, w2 = ff
        w2(rb, w1(rb, xn, act=ACT_RELU), act=ACT_NONE, alpha=scale, resid=x, out=x, out_f32=True)

    def _mha(self, rb, x, L, pos, kv_len=None):
        A, H, dk = self.A, self.H, self.dk
        xn = hip.layernorm(x, L["norm_mha"][0], L["norm_mha"][1], self.dtype, LN_EPS)
        vcol, ldvt = rb.vt_layout()
        if "qkv" in L:
            qk, vt = L["qkv"](rb, xn, split=(2 * A, ldvt, vcol))                             # (R, 2A), (A, ldvt)
        else:
            qk = L["qk"](rb, xn)                                                             # (R, 2A)
            vt = L["v"](rb, xn, transposed=True, out_ld=ldvt, y_seq_col0=vcol)               # (A, ldvt)
        g = ku = None
        ldg = 0
        rel_mode, rel_center = 1, 0
        if L["rel"]:
            cap, (heads, cv) = pos
            n_pos = cv.shape[1]                       # cap (legacy) or 2cap-1 (new)
            ldg = hip.round_up(n_pos, 32)
            if self.rel_style == "new":
                rel_mode, rel_center = 2, cap - 1
            ku = hip.rowdot(qk, 2 * A, rb.total, H, dk, L["u"], col0=A)                          # u . k_j
            g = torch.empty(rb.total, H * ldg, dtype=hip.torch_dtype(self.dtype), device=x.device)
            for h in range(H):  # g[row][h][m] = q_row,h . p_h[m] + v_h . p_h[m]
                hip.conv1d(rb, qk, heads[h], hip.round_up(dk, 64), n_pos, 1, dtype=self.dtype, bias=cv[h], ldx=2 * A,
                           x_col0=h * dk, out=g, out_ld=H * ldg, out_col0=h * ldg)
        ctx = hip.relpos_attention(rb, qk, 2 * A, qk, 2 * A, vt, ldvt, g, ldg, ku, 1.0 / math.sqrt(dk),
                                   H, dk, hip.attention_dtype(self.dtype, self.split, self.attn, H, dk, rel_mode), q_col0=0, k_col0=A, rel_mode=rel_mode, rel_center=rel_center, vt_col0=vcol,
                                   kv_len=kv_len)
        L["o"](rb, ctx, resid=x, out=x, out_f32=True)

    def _convmod(self, rb, x, L):
        xn = hip.layernorm(x, L["norm_conv"][0], L["norm_conv"][1], self.dtype, LN_EPS)
        pw = L["pw1"](rb, xn)
        dw = hip.glu_dwconv_bn_swish(rb, pw, self.A, L["dw_k"], L["dw_w"], L["dw_s"], L["dw_t"], self.dtype)
        L["pw2"](rb, dw, resid=x, out=x, out_f32=True)

    def run(self, rb, x, final_dtype=None, taps=None, kv_len=None):
        """x: f32 (rows, A) = input-layer output BEFORE the x*sqrt(A) scaling is applied by the caller.
        Returns after_norm output as f32 (or ``final_dtype``).  x is updated in place.
        kv_len (int32 device tensor, n_seq): key padding mask of a PADDED batch (the reference's batched forward():
        encoder.py:233-289 with masks) -- only the attention sees it, exactly as in the reference."""
        pos = self._pos(rb.max_len) if any(L["rel"] for L in self.layers) else None  # (cap, per_layer)
        for i, L in enumerate(self.layers):
            macaron = "feed_forward_macaron" in L
            ff_scale = 0.5 if macaron else 1.0
            if macaron:
                self._ffn(rb, x, L["norm_ff_macaron"], L["feed_forward_macaron"], ff_scale)
            self._mha(rb, x, L, (pos[0], pos[1][i]) if pos else None, kv_len)
            if "pw1" in L:
                self._convmod(rb, x, L)
            self._ffn(rb, x, L["norm_ff"], L["feed_forward"], ff_scale)
            if "norm_final" in L:
                hip.layernorm(x, L["norm_final"][0], L["norm_final"][1], hip.F32, LN_EPS, out=x)
            if taps is not None:
                taps[f"layer{i}"] = x.clone()
        if self.after_norm is None:
            return x
        od = hip.F32 if final_dtype is None else final_dtype
        return hip.layernorm(x, self.after_norm[0], self.after_norm[1], od, LN_EPS)
