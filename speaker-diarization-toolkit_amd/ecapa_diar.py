"""Diarize in the ECAPA space: the embedder diarize.Diarizer and stream.StreamBank read, on the engine's own ECAPA-TDNN.

The Diarizer reads four members off its embedding network: .cfg.embed_dim, .precision, .last_map_frames(T) and
.forward_masked(feats, B, T, w, valid).  resnet.ResNet34 has them; EcapaEmbedder gives them to the engine's ECAPA-TDNN (C = 1024), whose
weight blob it uses as it stands - trained-weight import, the bias correction and the enrolled profiles' space are shared, so the centroids
of a diarization can be scored against enrolled speakers (Backend.link_speakers(candidates=...)).

THE RULE (include/sdk_hip.h and csrc/asp_masked.hip state it in full; parity with SpeechBrain and PyAnnote is unpinned, the tests pin this):
for a chunk the trunk of sdk_ecapa_forward - blk0, the SE-Res2Net blocks, MFA, up to h [T, Cm] - runs once, bit for bit the values
sdk_ecapa_forward computes at the same (B, T); the SE squeeze stays over all T frames; the mask enters at the pooling only.  For each slot s,
w = w[b][s][0..T) >= 0 (any non-negative weights), v1 = sum w:
  context    mu = sum w h / v1,  sd = sqrt(max(sum w (h - mu)^2 / v1, 1e-12))
  ubias      Wms [mu | sd] + b (fp32), hidden a = tanh(BN(relu(h Wh + ubias))) in the 2-byte format, logits l = a . W2 + b2 (fp32)
  attention  m = max over {t : w_t > 0} of l,  e_t = w_t exp(l_t - m),  alpha = e / sum e  (a frame with w_t = 0 enters nothing)
  pooled     wmu = sum alpha h,  wsd = sqrt(max(sum alpha (h - wmu)^2, 1e-12));  embedding = fc(asp_bn(wmu | wsd))
A row depends on its own weights only; rows with valid == 0 are zeros; a row with valid != 0 and v1 <= 0 is ZEROED.  With w == 1 this is
the pooling of sdk_ecapa_forward, with 0 / 1 weights SpeechBrain's masked AttentiveStatisticsPooling.  There is no time down-sampling:
last_map_frames(T) is T, and sdk_diarize_masks maps the segmentation's F frames onto the T fbank frames by i(j) = min(F - 1, (j F) / T)."""
from __future__ import annotations


class EcapaEmbedder:
    """The engine's ECAPA-TDNN as a Diarizer's embedding network.  precision: the engine's at construction (0: bf16, or 2: fp16); the
    Diarizer switches the engine to it for a run and the caller gives it back, as with the ResNet34."""

    def __init__(self, engine, precision=None):
        self.eng = engine
        self.cfg = engine.cfg
        self.precision = int(engine.precision if precision is None else precision)
        if self.precision not in (0, 2):
            raise ValueError(f"EcapaEmbedder: precision {self.precision} is not served: the masked pooling is built for modes 0 (bf16) and 2 (fp16)")
        self.bias_correction = bool(engine.bias_correction)

    def last_map_frames(self, T: int) -> int:
        """Frames the pooling weights cover for chunks of T fbank frames: T (the TDNN trunk keeps every frame)."""
        return int(T)

    def forward_masked(self, feats, B: int, T: int, w, valid):
        """Engine.ecapa_forward_masked in this embedder's numerical contract: w [B, S, T] fp32, valid [B, S] int32 -> [B * S, embed_dim]."""
        if self.eng.precision != self.precision:
            self.eng.set_precision(self.precision)
        return self.eng.ecapa_forward_masked(feats, B, T, w, valid)
