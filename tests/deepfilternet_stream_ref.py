"""numpy reference of the DeepFilterNet hop-by-hop streamer (DeepFilterNetStreamer of the reference), float64 by default, written on the
layers of tests/deepfilternet_ref.py.  One hop at a time: analysis and synthesis memories, per-frame features with carried
normalisation states, fixed conv histories, the GRU step, the spec ring that reads zeros for frames not yet written, and, as
processChunk, neither the division by sum w^2 nor the clip.  Hop h makes frame h; once frame t + conv_lookahead exists, target t emits
hop_size samples (the first target's are the fft - hop samples of delay)."""
import numpy as np

import deepfilternet_ref as R


class DeepFilterNetStreamRef:
    def __init__(self, cfg, W, dtype=np.float64):
        self.ref = R.DeepFilterNetRef(cfg, W, dtype)
        self.cfg, self.d, self.W = cfg, self.ref.d, self.ref.W
        assert cfg.fft_size == 2 * cfg.hop_size and cfg.df_lookahead <= cfg.conv_lookahead
        self.reset()

    def kT(self, key):
        return self.W[key].shape[2]

    def reset(self):
        c, d = self.cfg, self.d
        E, D, C = c.nb_erb, c.nb_df, c.conv_ch
        self.hops = 0
        self.ana = np.zeros(c.fft_size - c.hop_size, d)                   # analysis memory
        self.syn = np.zeros(c.fft_size - c.hop_size, d)                   # synthesis memory (overlap-add tail)
        self.s_erb = R.linspace(-60.0, -90.0, E, d.type)
        self.s_df = R.linspace(0.001, 0.0001, D, d.type)
        self.h_erb0 = np.zeros((self.kT("enc.erb_conv0.1.weight") - 1, E, 1), d)      # fixed histories: kT - 1 input frames
        self.h_df0 = np.zeros((self.kT("enc.df_conv0.1.weight") - 1, D, 2), d)
        self.h_dfp = np.zeros((self.kT("df_dec.df_convp.1.weight") - 1, D, C), d)
        self.h = {}                                                       # (chain, layer) -> h
        self.ring = {}                                                    # absolute frame -> unmasked spec [2 F]; missing reads as zeros
        self.lsnr = []

    # -- one GRU step from the carried state
    def gru_step(self, x, p, l):
        d = self.d
        wih, whh = self.ref.w(f"{p}.gru.weight_ih_l{l}"), self.ref.w(f"{p}.gru.weight_hh_l{l}")
        bih, bhh = self.ref.w(f"{p}.gru.bias_ih_l{l}"), self.ref.w(f"{p}.gru.bias_hh_l{l}")
        H = whh.shape[1]
        h = self.h.get((p, l), np.zeros(H, d))
        gx, gh = x @ wih.T + bih, h @ whh.T + bhh
        r, z = R.sigmoid(gx[:H] + gh[:H]), R.sigmoid(gx[H: 2 * H] + gh[H: 2 * H])
        n = np.tanh(gx[2 * H:] + r * gh[2 * H:])
        h = (d.type(1) - z) * n + z * h
        self.h[(p, l)] = h
        return h

    def squeezed(self, x, p, out=True):
        y = self.ref.linear_in(x[None], p)[0]
        for l in range(R.n_layers(self.W, p)):
            y = self.gru_step(y, p, l)
        return self.ref.linear_out(y[None], p)[0] if out else y

    def last(self, hist, frame, fn):
        """A causal conv block on its fixed history + the new frame: the last output row; returns it and the history moved on."""
        win = np.concatenate([hist, frame[None]])
        return fn(win)[-1:], win[1:]

    def hop(self, x):
        """hop_size samples -> hop_size output samples, or None while the look-ahead fills."""
        c, r, d = self.cfg, self.ref, self.d
        F, D, L = c.freq_bins, c.nb_df, c.conv_lookahead
        x = np.asarray(x, d)
        fr = np.concatenate([self.ana, x]) * r.win
        self.ana = x[len(x) - len(self.ana):] if len(self.ana) <= len(x) else np.concatenate([self.ana, x])[-len(self.ana):]
        s = (r._rfft32(fr[None])[0] if d == np.float32 else np.fft.rfft(fr)) * r.wnorm
        spec = np.concatenate([s.real, s.imag]).astype(d)
        k = self.hops
        self.hops += 1
        self.ring[k] = spec
        # features of frame k with the carried states
        a, oma = d.type(r.alpha), d.type(1) - d.type(r.alpha)
        e = r.erb_db(spec[None])[0]
        self.s_erb = e * oma + self.s_erb * a
        f_erb = ((e - self.s_erb) / d.type(40))[:, None]
        re, im = spec[:D], spec[F: F + D]
        self.s_df = np.sqrt(re * re + im * im) * oma + self.s_df * a
        den = np.sqrt(np.maximum(self.s_df, d.type(1e-12)))
        f_df = np.stack([re / den, im / den], axis=-1)
        t = k - L                                                         # the target whose shifted input is frame k
        if t < 0:
            return None
        e0, self.h_erb0 = self.last(self.h_erb0, f_erb, lambda w: r.block(w, "enc.erb_conv0", 1, None, 2))
        e1 = r.e1(e0); e2 = r.e2(e1); e3 = r.e3(e2)
        c0, self.h_df0 = self.last(self.h_df0, f_df, lambda w: r.block(w, "enc.df_conv0", 1, 2, 3))
        c1 = r.c1(c0)
        emb = self.squeezed(r.emb0(e3, c1)[0], "enc.emb_gru")
        self.lsnr.append(r.lsnr(emb[None])[0])
        embd = self.squeezed(emb, "erb_dec.emb_gru")
        d3 = r.d3(r.pathway(e3, 3, embd.reshape(e3.shape)))
        d2 = r.d2(r.pathway(e2, 2, d3))
        d1 = r.d1(r.pathway(e1, 1, d2))
        mask = r.mask(r.pathway(e0, 0, d1))
        cdf = r.df_skip(self.squeezed(emb, "df_dec.df_gru", out=False)[None], emb[None])
        c0p, self.h_dfp = self.last(self.h_dfp, c0[0], lambda w: r.c0p(w))
        coefs = r.coefs(cdf, c0p).reshape(D, c.df_order, 2)
        # synthesis of frame t: mask above nb_df, the deep filter over the ring below it
        cur = self.ring[t]
        gains = mask.reshape(1, -1) @ r.w("mask.erb_inv_fb")
        ore, oim = cur[:F] * gains[0], cur[F:] * gains[0]
        fr_, fi_ = np.zeros(D, d), np.zeros(D, d)
        pl = c.df_order - 1 - c.df_lookahead
        for j in range(c.df_order):
            sp = self.ring.get(t + j - pl)
            if sp is None:
                continue
            sr, si, cr, ci = sp[:D], sp[F: F + D], coefs[:, j, 0], coefs[:, j, 1]
            fr_, fi_ = fr_ + (sr * cr - si * ci), fi_ + (sr * ci + si * cr)
        ore[:D], oim[:D] = fr_, fi_
        self.ring.pop(t - pl - 1, None)
        enh = (np.concatenate([ore, oim]) / r.wnorm).astype(d)
        if d == np.float32:
            y = r._irfft32(enh[None])[0] * r.win
        else:
            y = np.fft.irfft(enh[:F] + 1j * enh[F:], n=c.fft_size) * r.win
        out = y[: c.hop_size] + self.syn
        self.syn = y[c.hop_size:]
        return out.astype(d)


def stream_all(st, x, pad_end_frames=0):
    """Every whole hop of x (+ the end padding), the remainder dropped: the raw concatenation, the delay in front included."""
    hop = st.cfg.hop_size
    x = np.concatenate([np.asarray(x, st.d), np.zeros(pad_end_frames * hop, st.d)])
    outs = [st.hop(x[h * hop: (h + 1) * hop]) for h in range(len(x) // hop)]
    outs = [o for o in outs if o is not None]
    return np.concatenate(outs) if outs else np.zeros(0, st.d)
