"""What the two families of drop-in explainers - `ExplainGridTDAttention` (explainers/gridtd.py) and `ExplainAOAAttention`
(explainers/aoa.py) with their four gradient-family subclasses each - share: the engine lookup, image preprocessing, the caption
bookkeeping of `get_hidden_parameters`, `explain_cnn`, `teacherforce_forward` and the tail of `explain_caption`.

Conventions of both families: `model` may be the reference's model (any nn.Module with that `state_dict`), a `state_dict`, or None
(then `args.weight` is loaded as the reference does).  Wherever the reference takes a file path a (1,3,H,W) tensor is accepted too.
Without `caption_encode=` the image is captioned by the reference's own procedure (the engine's `beam_search`), so the same caption is
explained.  Nothing is written to disk (visualisation is out of scope)."""
import numpy as np
import torch

from .. import _lib, ops
from .._lib import check, ptr, stream_ptr

IMAGENET_MEAN, IMAGENET_STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


def load_image(img_filepath, height, width, mean, std, device):
    """`preprocess_img` of every reference explainer (models/gridTDmodel.py:767-771, models/aoamodel.py:864-868): PIL open ->
    RGB -> `transforms.Resize((height, width))` (PIL bilinear) -> `ToTensor` (/255, CHW) -> `Normalize(mean, std)` -> (1,3,H,W)
    on the device.  Host side, as in the reference (image decoding is outside the path)."""
    from PIL import Image
    im = Image.open(img_filepath).convert('RGB').resize((width, height), Image.BILINEAR)
    x = torch.from_numpy(np.asarray(im, dtype=np.float32) / 255.0).permute(2, 0, 1)
    x = (x - torch.tensor(mean).view(3, 1, 1)) / torch.tensor(std).view(3, 1, 1)
    return x.unsqueeze(0).contiguous().to(device)


class ExplainerBase(object):
    """Attributes after `get_hidden_parameters` / `explain_caption`: `.model .word_map .args .img .img_filepath .beam_caption
    .beam_caption_encode .caption_length .num_pixels`, and for a caption that is not empty `.predictions .alphas .image_features`
    (`.betas` where the trace has a sentinel gate)."""
    EPS = 0.01
    EX_TYPE = 'lrp'
    TF_MODEL_BIAS = False      # the LRP explainers' LanguageLSTM forward adds bias_ih twice (gridTDmodel.py:789, aoamodel.py:873); the gradient families' is correct
    _RUNNING_SUMS = True       # `explain_caption` / `explain_cnn` return running sums over the words (`sample.grad`, lrp_wrapper.py:64-82): LRP only

    # ---- hooks -------------------------------------------------------------------------------------------------------------------------
    def _engine_key(self):
        """the engine_cache key of this explainer's weights (explainers/engine_cache.py: `fingerprint`)"""
        raise NotImplementedError

    def _build_engine(self, state):
        raise NotImplementedError

    def _accept_engine(self, engine):
        """refuse an engine this class cannot explain on (before a replica is taken)"""

    def _explain_rows(self, head_idx):
        """the decoder's explanation of every word of the traced caption: (feat (T,P,C), r_words (T,T), row2img)"""
        raise NotImplementedError

    def _cnn(self, feat_nhwc, row2img):
        """the encoder stage: (rows,P,C) at the encoder's features -> maps, under this explainer's `lrp_params` (None: the preset;
        explainers/engine_base.py: `_maps_stage`).  The value is passed, never written to the engine: engines are shared."""
        return self.engine._maps_stage("explain_cnn", getattr(self, "lrp_params", None))(feat_nhwc, row2img)

    # ---- shared --------------------------------------------------------------------------------------------------------------------------
    def __init__(self, args, word_map, model=None):
        self.args = args
        self.word_map = word_map
        self.vocab_size = len(word_map)
        self.model = model
        self.lrp_params = None          # {"alpha": 2., "beta": 1.}: the Conv2d rule of `explain_cnn` (LRP explainers; None: the preset)
        from . import engine_cache

        def build():
            if model is None:
                state = torch.load(args.weight, map_location="cpu")['state_dict']
            elif hasattr(model, "state_dict"):
                state = model.state_dict()
            else:
                state = model
            return self._build_engine(state)
        # one device engine per weight set (explainers/engine_cache.py): evaluation.py:806-838 builds an explainer per image.  The weights
        # are shared, the trace / workspace buffers are this explainer's own: two live explainers never see each other's image (the state
        # dict of a model holds its encoder's tensors too: key and `hold` cover the module as they cover the state)
        engine = engine_cache.get(self._engine_key(), build, hold=engine_cache.source_tensors(model))
        self._accept_engine(engine)
        self.engine = engine.replica()
        self.mean = list(IMAGENET_MEAN)
        self.std = list(IMAGENET_STD)
        self.rev_word_map = {v: k for k, v in word_map.items()}

    def preprocess_img(self, img_filepath):
        """Resize -> ToTensor -> Normalize (models/gridTDmodel.py:767-771, models/aoamodel.py:864-868), host side."""
        return load_image(img_filepath, getattr(self.args, "height", 224), getattr(self.args, "width", 224), self.mean, self.std,
                          self.engine.device)

    def _hidden_parameters(self, img, caption_encode, beam_size, max_cap_length):
        """Forward trace of `get_hidden_parameters`.  `img`: file path or a (1,3,H,W) tensor of the encoder's image size."""
        eng = self.engine
        if isinstance(img, str):
            self.img_filepath = img
            self.img = self.preprocess_img(img)
        else:
            self.img = img.to(eng.device, torch.float32)
        # a caption that is handed over goes to the device BEFORE the encoder is enqueued: the copy of a pageable host list waits for the
        # stream, and behind the VGG16 forward it stalled the host for 1 ms per call (the device then idled until the decoder was issued)
        cap_dev = None if caption_encode is None else torch.tensor([[int(c) for c in caption_encode]], dtype=torch.int64, device=eng.device)
        self._enc = eng.encode(self.img)
        if caption_encode is None:
            from .beam import caption_from_sequence
            seq = eng.beam_search(self._enc, beam_size, max_cap_length, self.word_map['<start>'], self.word_map['<end>'])
            caption_encode = caption_from_sequence(seq, self.word_map)
        self.beam_caption_encode = [int(c) for c in caption_encode]
        special = {self.word_map[k] for k in ('<start>', '<end>', '<unk>', '<pad>') if k in self.word_map}
        self.beam_caption = [' '.join(self.rev_word_map.get(c, str(c)) for c in self.beam_caption_encode[1:]
                                      if c not in special)]
        self.caption_length = len(self.beam_caption_encode) - 1
        self.num_pixels = self._enc["feats"].shape[1]
        self._rel = {}
        if self.caption_length == 0:
            return
        self._cap_dev = cap_dev if cap_dev is not None else torch.tensor([self.beam_caption_encode], dtype=torch.int64, device=eng.device)
        self._trace(grad=False)
        self.image_features = ops.nhwc_to_nchw(self._enc["feats"].contiguous(), eng.C, *eng.cnn.feat_hw)

    def _trace(self, grad):
        """grad=True: the gradient families' trace (correct LSTM bias, output gates kept)"""
        self._tr = self.engine.trace(self._enc, self._cap_dev, predictions=True, grad=grad)
        self.predictions = self._tr["pred"][0]
        self.alphas = self._tr["alpha"][0]
        if "beta" in self._tr:
            self.betas = self._tr["beta"][0]

    def _relevance(self, head_idx=None):
        if head_idx not in self._rel:
            self._rel[head_idx] = self._explain_rows(head_idx)
        return self._rel[head_idx]

    def _explain_wordt(self, t, head_idx=None):
        """-> (r_img_feature (1,C,h,w), r_words (t+1,))"""
        assert t < self.caption_length
        r_feat, r_words, _ = self._relevance(head_idx)
        return ops.nhwc_to_nchw(r_feat[t:t + 1].contiguous(), self.engine.C, *self.engine.cnn.feat_hw), r_words[t, :t + 1].clone()

    def _one_map(self, img_feature):
        """(n,C,h,w) at the encoder's features -> what `_cnn` takes: NHWC rows, all of image 0"""
        return ops.nchw_to_nhwc(img_feature.to(torch.float32)), torch.zeros(img_feature.shape[0], dtype=torch.int32, device=self.engine.device)

    def explain_cnn(self, r_img_feature):
        """(models/gridTDmodel.py:1137-1139, models/aoamodel.py:1158-1160) the encoder stage on `self.img`.  LRP (`compute_lrp`): like the
        reference the result accumulates over calls on the same image (`sample.grad`, lrp_wrapper.py:64-82)."""
        r = self._cnn(*self._one_map(r_img_feature))
        if not self._RUNNING_SUMS:
            return r
        if getattr(self, "_img_grad", None) is None:
            self._img_grad = r
        else:
            check(_lib.load().lrpx_accumulate(ptr(self._img_grad), ptr(r), r.numel(), stream_ptr()))
        ops.check_relevance(self._img_grad, finite=True, nonzero=True)
        return self._img_grad.clone()

    def _explain_caption(self, img_filepath, caption_encode, head_idx=None):
        """-> ([T] x maps (1,...), [T] x r_words (t+1,)); LRP: the maps are the reference's running sums"""
        self.img_filepath = img_filepath
        self.get_hidden_parameters(img_filepath, caption_encode)
        if self.caption_length == 0:          # the beam search produced <end> first: nothing to explain (empty lists)
            return [], []
        feat, r_words, row2img = self._relevance(head_idx)
        maps = self._cnn(feat, row2img)
        if self._RUNNING_SUMS:
            self._img_grad = None
            maps = ops.cumsum_maps(maps, 1, self.caption_length)
            ops.check_relevance(maps, finite=True, nonzero=True)
        return ([maps[t:t + 1] for t in range(self.caption_length)],
                [r_words[t, :t + 1] for t in range(self.caption_length)])

    def teacherforce_forward(self, img, beam_caption_encode):
        """(models/gridTDmodel.py:892-931, gradient family :1282-1321; models/aoamodel.py:952-988, :1377-1413) -> predictions
        (len(beam_caption_encode), V) under teacher forcing: step t reads token t - evaluation.py:266,437,702,767 hand the caption WITH
        <start> - with this explainer's own LanguageLSTM forward (`TF_MODEL_BIAS`)."""
        eng = self.engine
        if isinstance(img, str):
            img = self.preprocess_img(img)
        enc = eng.encode(img.to(eng.device, torch.float32))
        cap = torch.tensor([[int(c) for c in beam_caption_encode] + [0]], dtype=torch.int64, device=eng.device)
        n = cap.shape[1] - 1
        tr = eng.trace(enc, cap, model_bias=self.TF_MODEL_BIAS, predictions=False)
        return eng.logits(tr["hc"].view(n, eng.H))       # the fp32 kernel of the decoding loops, at any caption length
