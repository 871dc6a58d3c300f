"""model/defineModel.py of the reference: Backbone / ResNetBackbone, the submodel and pyramid builders, retinanet,
retinanet_bbox and the resnet*_retinanet constructors (model/defineModel.py:9-402) — returning a Model object with the Keras
methods RetinaNet.py uses (compile, fit_generator, train_on_batch, predict_on_batch, load_weights, save, get_layer, ...),
executed by the HIP engine.  Weight files are .npz with the reference checkpoint's layer names ('<layer>/kernel' HWIO ...);
Keras HDF5 import needs h5py, which this image lacks."""
import os

import numpy as np
import torch

from . import _rt, initializers, layers, losses, utils
from .anchors import AnchorParameters_default

Wt = _rt.weights


class _LayerRef:
    def __init__(self, name, kind):
        self.name, self.kind, self.trainable = name, kind, True
        self.output = "%s:output" % name


def is_backbone_layer(name):
    """The ResNet's own conv layers (keras_resnet's model): conv1 and res*.  The FPN (C*_reduced, P*) and the heads (pyramid_*) are
    not."""
    return name == "conv1" or name.startswith("res")


class BackboneView:
    """The ResNet backbone of a Model as the reference's `modifier` sees it (model/defineModel.py:384-386: freeze_model is applied to
    the keras_resnet model only): `.layers` are the Model's own conv1 / res* layer objects, so a modifier that sets `trainable`
    on them freezes exactly the backbone."""

    def __init__(self, model):
        self.model = model
        self.name = model.backbone
        self.layers = [l for l in model.layers if l.kind == "conv" and is_backbone_layer(l.name)]

    def get_layer(self, name):
        for l in self.layers:
            if l.name == name:
                return l
        raise ValueError('No such layer: ' + name)


class Adam:
    """ keras.optimizers.Adam(lr, clipnorm) stand-in accepted by Model.compile (RetinaNet.py:130).  `clipnorm` clips by the GLOBAL
    gradient norm (standalone Keras 2.x, the reference's `import keras`); global_clipnorm=False selects the per-tensor
    tf.clip_by_norm of tf.keras / Keras >= 2.4."""

    def __init__(self, lr=0.001, beta_1=0.9, beta_2=0.999, epsilon=1e-7, clipnorm=None, global_clipnorm=True, **kwargs):
        self.lr, self.beta_1, self.beta_2, self.epsilon, self.clipnorm = lr, beta_1, beta_2, epsilon, clipnorm
        self.global_clipnorm = bool(global_clipnorm)


class History:
    def __init__(self):
        self.history = {}


class Model:
    """The training model (outputs [regression, classification]) or, with bbox=True, the inference model
    (outputs [boxes, scores, labels])."""

    def __init__(self, backbone, num_classes, num_anchors, name='retinanet', bbox=False, base=None, anchor_params=None,
                 dtype=None, seed=0, nms=True, class_specific_filter=True):
        self.backbone, self.num_classes, self.num_anchors, self.name = backbone, num_classes, num_anchors, name
        self.bbox, self.base = bbox, base
        self.nms, self.class_specific_filter = bool(nms), bool(class_specific_filter)   # FilterDetections' switches (bbox=True)
        self.anchor_params = anchor_params
        self.dtype = dtype or os.environ.get("RTN_DTYPE", "bf16")
        self.inputs = ["input_1"]
        self.output_names = ['filtered_detections'] * 3 if bbox else ['regression', 'classification']
        self.outputs = ["boxes", "scores", "labels"] if bbox else ["regression", "classification"]
        self.layers = [_LayerRef("input_1", "input")] + [_LayerRef(n, "conv") for (n, *_r) in Wt.conv_layers(backbone, num_classes, num_anchors)]
        self.layers += [_LayerRef(n, "merge") for n in ("regression", "classification")]
        self.stop_training = False
        self._state = base._state if base is not None else Wt.init_state(backbone, num_classes, num_anchors, seed=seed)
        self._engine = None
        self._trainer = None
        self._compiled = None

    # ---- Keras surface
    def get_layer(self, name):
        for l in self.layers:
            if l.name == name:
                return l
        if name in ("P3", "P4", "P5", "P6", "P7"):
            return _LayerRef(name, "conv")
        raise ValueError('No such layer: ' + name)

    def _root(self):
        return self.base._root() if self.base is not None else self

    def engine(self):
        root = self._root()
        if root._engine is None:
            ap = None
            if self.anchor_params is not None:
                ap = _rt.engine.AnchorParams(self.anchor_params.sizes, self.anchor_params.strides, self.anchor_params.ratios,
                                             self.anchor_params.scales)
            root._engine = _rt.engine.Engine(root.backbone, root.num_classes, root.num_anchors, dtype=root.dtype, anchor_params=ap)
            root._engine.load_state(root._state)
        return root._engine

    def compile(self, loss=None, optimizer=None, **kwargs):
        if loss is not None and set(loss) != {'regression', 'classification'}:
            raise ValueError("loss must name the 'regression' and 'classification' outputs")
        self._compiled = optimizer if optimizer is not None else Adam(lr=1e-4, clipnorm=0.001)
        root = self._root()
        if root._trainer is not None:                             # Keras: `trainable` changes take effect at compile()
            root._trainer.set_trainable(root._trainable_names())

    def backbone_view(self):
        """The ResNet part of this model (BackboneView): what resnet_retinanet(modifier=...) hands the modifier."""
        return BackboneView(self._root())

    def _trainable_names(self):
        """None when every conv layer trains (the full backward), else the set of trainable conv layers."""
        convs = [l for l in self._root().layers if l.kind == "conv"]
        if all(l.trainable for l in convs):
            return None
        return frozenset(l.name for l in convs if l.trainable)

    def _get_trainer(self):
        root = self._root()
        if root._trainer is None:
            opt = self._compiled or Adam(lr=1e-4, clipnorm=0.001)
            pg = None
            if torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1:
                pg = torch.distributed.group.WORLD
            # utils.freeze / freeze_model: non-trainable layers get no gradient and no update (Trainer(trainable=...))
            root._trainer = _rt.trainer.Trainer(self.engine(), lr=opt.lr, clipnorm=(opt.clipnorm or 0.0), beta1=opt.beta_1,
                                                beta2=opt.beta_2, eps=opt.epsilon, process_group=pg,
                                                global_clip=getattr(opt, "global_clipnorm", True), trainable=root._trainable_names())
        return root._trainer

    def predict_on_batch(self, x):
        x = _rt.dev(x, torch.float32) if not (isinstance(x, np.ndarray) and x.dtype == np.uint8) else _rt.dev(x, torch.uint8)
        eng = self.engine()
        if self.bbox:
            b, s, l = eng.detect(x, nms=self.nms, class_specific_filter=self.class_specific_filter)
            return [_rt.host(b).copy(), _rt.host(s).copy(), _rt.host(l).copy()]
        r, c = eng.forward(x)
        return [_rt.host(r).copy(), _rt.host(c).copy()]

    predict = predict_on_batch

    def predict_generator(self, generator, steps=None, in_flight=2, **kwargs):
        """keras.Model.predict_generator for the inference model (retinanet_bbox, model/defineModel.py:296-353): the batches of
        `generator` (a Sequence - generator[i] -> inputs or (inputs, targets) - or any iterable of them) run with `in_flight`
        batches on the device at a time (Engine.in_flight: the next batch's backbone fills the CUs the current batch's small layers
        leave idle, + 15 % pages per second at batch 8); every batch's [boxes, scores, labels] are copied out as soon as THAT batch
        is done.  Returns the three arrays concatenated over the batches (Keras semantics).  RetinaNet.py's test() calls
        predict_on_batch page by page; a caller with many pages gets this instead."""
        if not self.bbox:
            raise ValueError("predict_generator: the inference model (retinanet_bbox) - the training model's outputs go through predict_on_batch")
        from collections import deque
        eng = self.engine()
        n = len(generator) if (steps is None and hasattr(generator, "__len__")) else steps
        it = (generator[i] for i in range(n)) if hasattr(generator, "__getitem__") and n is not None else iter(generator)
        outs, pending = ([], [], []), deque()
        modes = {"nms": self.nms, "class_specific_filter": self.class_specific_filter}

        def fetch():
            slot, views = pending.popleft()
            eng.wait_slot(slot)
            for o, v in zip(outs, views):
                o.append(_rt.host(v).copy())
        prev = eng.in_flight
        eng.join()
        eng.in_flight = max(1, int(in_flight))
        try:
            for k, item in enumerate(it):
                if n is not None and k >= n:
                    break
                x = item[0] if isinstance(item, (tuple, list)) else item
                x = _rt.dev(x, torch.float32) if not (isinstance(x, np.ndarray) and x.dtype == np.uint8) else _rt.dev(x, torch.uint8)
                if eng.in_flight == 1:
                    views = eng.detect(x, **modes)
                    torch.cuda.current_stream().synchronize()
                    for o, v in zip(outs, views):
                        o.append(_rt.host(v).copy())
                    continue
                if len(pending) == eng.in_flight:            # its buffer set is the one the next call rewrites
                    fetch()
                views = eng.detect(x, **modes)
                pending.append((eng.last_slot, views))
            while pending:
                fetch()
        finally:
            eng.join()
            eng.in_flight = prev
        return [np.concatenate(o, axis=0) if o else np.zeros((0,)) for o in outs]

    def train_on_batch(self, x, y):
        tr = self._get_trainer()
        total, reg, cls = tr.train_on_batch(_rt.dev(x, torch.float32), _rt.dev(y[0], torch.float32), _rt.dev(y[1], torch.float32),
                                            lr=getattr(self._compiled, "lr", None))
        return [total, reg, cls]

    @property
    def optimizer(self):
        """The compiled optimizer (keras.Model.optimizer): callbacks read and set its `lr`, which every training step picks up."""
        if self._compiled is None:
            self._compiled = Adam(lr=1e-4, clipnorm=0.001)
        return self._compiled

    def _loss_sums(self, x, y):
        """One forward of the training model and ONE rtn_retina_loss_fwd on its outputs against the dense targets
        y = [regression_batch (B,N,5), labels_batch (B,N,K+1)]: the device f64 {focal sum, smooth-L1 sum, positives, positives}.
        The outputs never leave the device."""
        if self.bbox:
            raise ValueError("test_on_batch: the training model's outputs are needed (this is the inference model)")
        x = _rt.dev(x, torch.float32) if not (isinstance(x, np.ndarray) and x.dtype == np.uint8) else _rt.dev(x, torch.uint8)
        reg, cls = self.engine().forward(x)
        regt, lab = _rt.dev(y[0], torch.float32), _rt.dev(y[1], torch.float32)
        B, N, K = cls.shape
        if tuple(regt.shape) != (B, N, 5) or tuple(lab.shape) != (B, N, K + 1):
            raise ValueError("targets (%d,%d,5) and (%d,%d,%d) expected, got %s and %s"
                             % (B, N, B, N, K + 1, tuple(regt.shape), tuple(lab.shape)))
        h = _rt.handle()
        wsb = _rt.L.lib.rtn_retina_loss_workspace_bytes(B * N)
        ws = torch.empty(wsb, dtype=torch.uint8, device=cls.device)
        sums = torch.zeros(4, dtype=torch.float64, device=cls.device)
        h.check(_rt.L.lib.rtn_retina_loss_fwd(h.raw, B * N, K, lab.data_ptr(), regt.data_ptr(), cls.data_ptr(), reg.data_ptr(),
                                              0.25, 2.0, 3.0, sums.data_ptr(), ws.data_ptr(), wsb))     # the functors' defaults
        return sums

    @staticmethod
    def _losses_of(s):
        """[regression_loss, classification_loss] of four sums, as the functors of model/losses.py round them (float32)."""
        return [float(np.float32(s[1] / max(1.0, s[3]))), float(np.float32(s[0] / max(1.0, s[2])))]

    def test_on_batch(self, x, y):
        """keras.Model.test_on_batch for the compiled pair of losses: [loss, regression_loss, classification_loss].  Each part has
        the bits of losses.smooth_l1()(y[0], regression) / losses.focal()(y[1], classification) on the same outputs (one launch
        computes both halves; the halves do not mix); loss is their sum."""
        reg, cls = self._losses_of(_rt.host(self._loss_sums(x, y)))
        return [reg + cls, reg, cls]

    def _test_batches(self, batches):
        """test_on_batch over an iterable of (x, y) with one read-back for all of them: [(batch size, regression_loss,
        classification_loss)]."""
        sizes, sums = [], []
        for x, y in batches:
            sums.append(self._loss_sums(x, y))
            sizes.append(int(y[0].shape[0]))
        if not sums:
            return []
        s = _rt.host(torch.stack(sums))
        return [(n,) + tuple(self._losses_of(row)) for n, row in zip(sizes, s)]

    def evaluate_generator(self, generator, steps=None, **kwargs):
        """keras.Model.evaluate_generator: [loss, regression_loss, classification_loss] over `steps` batches of a Sequence
        (default: all of it), each batch through test_on_batch's path, averaged with the batch sizes as weights (Keras:
        np.average(outs, weights=batch_sizes))."""
        n = len(generator) if steps is None else int(steps)
        per = self._test_batches(generator[j % len(generator)] for j in range(n))
        if not per:
            raise ValueError("evaluate_generator: no batches")
        w = np.asarray([p[0] for p in per], np.float64)
        reg = float(np.average([p[1] for p in per], weights=w))
        cls = float(np.average([p[2] for p in per], weights=w))
        return [reg + cls, reg, cls]

    def fit_generator(self, generator, steps_per_epoch=None, epochs=1, verbose=1, callbacks=None, validation_data=None,
                      workers=1, use_multiprocessing=False, max_queue_size=10, shuffle=True, initial_epoch=0, **kwargs):
        """ RetinaNet.py:280-291: Sequence-style generator (generator[i] -> (inputs, [regression_batch, labels_batch])).
        Callbacks (model/callbacks.py, model/customCallbacks.py, or any object with some of the hooks) are called in list order:
        set_model, on_train_begin, per epoch on_epoch_begin / on_epoch_end(epoch, logs), on_train_end; training stops after the
        epoch in which one of them sets `stop_training`."""
        from .callbacks import LearningRateScheduler
        hist = History()
        callbacks = callbacks or []
        steps = steps_per_epoch or len(generator)
        if self._compiled is None:                                # fit without compile(): the defaults _get_trainer would take
            self._compiled = Adam(lr=1e-4, clipnorm=0.001)
        self.stop_training = False
        for cb in callbacks:
            if hasattr(cb, "set_model"):
                cb.set_model(self)
        for cb in callbacks:
            if hasattr(cb, "on_train_begin"):
                cb.on_train_begin({})
        for epoch in range(initial_epoch, epochs):
            for cb in callbacks:
                if hasattr(cb, "on_epoch_begin"):
                    cb.on_epoch_begin(epoch, {})
                # LearningRateScheduler(lr_schedule), RetinaNet.py:47-66: a foreign object with a `.schedule`; the package's own
                # class has set the rate in its on_epoch_begin already
                if hasattr(cb, "schedule") and not isinstance(cb, LearningRateScheduler):
                    self._compiled.lr = cb.schedule(epoch)
            sums = np.zeros(3)
            for i in range(steps):
                x, y = generator[i % len(generator)]
                sums += np.array(self.train_on_batch(x, y))
            logs = dict(zip(("loss", "regression_loss", "classification_loss"), (sums / steps).tolist()))
            if validation_data is not None:
                v = np.zeros(3)
                for _, reg, cls in self._test_batches(validation_data[j] for j in range(len(validation_data))):
                    v += np.array([0.0, reg, cls])
                v /= max(1, len(validation_data))
                v[0] = v[1] + v[2]
                logs.update(dict(zip(("val_loss", "val_regression_loss", "val_classification_loss"), v.tolist())))
            for k, val in logs.items():
                hist.history.setdefault(k, []).append(val)
            if verbose:
                print("Epoch %d/%d - " % (epoch + 1, epochs) + " - ".join("%s: %.4f" % kv for kv in logs.items()))
            for cb in callbacks:
                if hasattr(cb, "on_epoch_end"):
                    cb.on_epoch_end(epoch, logs)
            if self.stop_training:
                break
        for cb in callbacks:
            if hasattr(cb, "on_train_end"):
                cb.on_train_end({})
        return hist

    # ---- weights
    def get_state(self):
        root = self._root()
        if root._trainer is not None:                               # pull the trained master weights back into Keras layout
            trained = root._trainer.get_state()
            root._state.update((k, v) for k, v in trained.items() if k.endswith(("/kernel", "/bias")))
        return root._state

    def save_weights(self, path):
        """Keras layer names and layouts either way: '*.h5' / '*.hdf5' -> a Keras save_weights() HDF5 file written by keras_h5.py
        (RetinaNet.py:70-79,153-163 save .h5), anything else -> .npz."""
        if str(path).endswith((".h5", ".hdf5")):
            _rt.keras_h5.save_keras_weights(path, self.get_state())
        else:
            np.savez(path, **self.get_state())

    save = save_weights

    def load_weights(self, path, by_name=True, skip_mismatch=False):
        root = self._root()
        if str(path).endswith((".h5", ".hdf5")):             # RetinaNet.py:320-340 loads training-*.h5 / inferModel.h5
            data = _rt.keras_h5.load_keras_state(path)
            names = list(data)
        else:
            data = np.load(path, allow_pickle=False)
            names = data.files
        for k in names:
            if k in root._state:
                if root._state[k].shape != data[k].shape:
                    if skip_mismatch:
                        continue
                    raise ValueError("shape mismatch for %s: %s vs %s" % (k, root._state[k].shape, data[k].shape))
                root._state[k] = data[k]
        if root._engine is not None:
            root._engine.load_state(root._state)
        root._trainer = None

    def summary(self):
        print("Model %s: %s, %d classes, %d anchors/cell" % (self.name, self.backbone, self.num_classes, self.num_anchors))


def load_model(path, custom_objects=None, backbone="resnet50", num_classes=1, num_anchors=9):
    m = Model(backbone, num_classes, num_anchors)
    m.load_weights(path)
    return m


class Backbone:
    """ Stores additional information on backbones (model/defineModel.py:9-48)."""

    def __init__(self, backbone):
        self.custom_objects = {
            'UpsampleLike': layers.UpsampleLike,
            'PriorProbability': initializers.PriorProbability,
            'RegressBoxes': layers.RegressBoxes,
            'FilterDetections': layers.FilterDetections,
            'Anchors': layers.Anchors,
            'ClipBoxes': layers.ClipBoxes,
            '_smooth_l1': losses.smooth_l1(),
            '_focal': losses.focal(),
        }
        self.backbone = backbone
        self.validate()

    def retinanet(self, *args, **kwargs):
        raise NotImplementedError('retinanet method not implemented.')

    def download_imagenet(self):
        raise NotImplementedError('download_imagenet method not implemented.')

    def validate(self):
        raise NotImplementedError('validate method not implemented.')

    def preprocess_image(self, inputs):
        raise NotImplementedError('preprocess_image method not implemented.')


class ResNetBackbone(Backbone):
    """ model/defineModel.py:50-75."""

    def retinanet(self, *args, **kwargs):
        return resnet_retinanet(*args, backbone=self.backbone, **kwargs)

    def validate(self):
        allowed_backbones = ['resnet50', 'resnet101', 'resnet152']
        backbone = self.backbone.split('_')[0]
        if backbone not in allowed_backbones:
            raise ValueError('Backbone (\'{}\') not in allowed backbones ({}).'.format(backbone, allowed_backbones))

    def preprocess_image(self, inputs):
        return utils.preprocess_image(inputs, mode='custom_tf')


def default_classification_model(num_classes, num_anchors, pyramid_feature_size=256, prior_probability=0.01,
                                 classification_feature_size=256, name='classification_submodel'):
    """ model/defineModel.py:78-125: descriptor of the 4 x (3x3, ReLU) + 3x3 -> sigmoid stack the engine executes."""
    return {"name": name, "prefix": "pyramid_classification", "outputs": num_classes * num_anchors, "activation": "sigmoid",
            "prior_probability": prior_probability, "feature_size": classification_feature_size}


def default_regression_model(num_values, num_anchors, pyramid_feature_size=256, regression_feature_size=256, name='regression_submodel'):
    """ model/defineModel.py:128-167."""
    return {"name": name, "prefix": "pyramid_regression", "outputs": num_values * num_anchors, "activation": None,
            "feature_size": regression_feature_size}


def retinanet(inputs, backbone_layers, num_classes, num_anchors=None, create_pyramid_features=None, submodels=None, name='retinanet',
              backbone='resnet50'):
    """ model/defineModel.py:232-267: outputs [regression, classification]."""
    if num_anchors is None:
        num_anchors = AnchorParameters_default.num_anchors()
    if create_pyramid_features is not None or submodels is not None:
        raise NotImplementedError("custom pyramid builders / submodels are not executed by the HIP engine")
    return Model(backbone, num_classes, num_anchors, name=name)


def retinanet_bbox(model=None, applyNms=None, class_specific_filter=True, name='retinanet-bbox', anchor_params=None, nms=None,
                   **kwargs):
    """ model/defineModel.py:296-353: appends Anchors -> RegressBoxes -> ClipBoxes -> FilterDetections; outputs
    [boxes, scores, labels].  applyNms (default True) and class_specific_filter are FilterDetections' two switches
    (model/layers.py:200-264); `nms` is keras-retinanet's spelling of applyNms and may be given instead of it."""
    if applyNms is not None and nms is not None and bool(applyNms) != bool(nms):
        raise ValueError("retinanet_bbox: applyNms=%r and nms=%r disagree" % (applyNms, nms))
    apply_nms = applyNms if applyNms is not None else (nms if nms is not None else True)
    if anchor_params is None:
        anchor_params = AnchorParameters_default
    if model is None:
        model = retinanet(num_anchors=anchor_params.num_anchors(), **kwargs)
    else:
        utils.assert_training_model(model)
    return Model(model.backbone, model.num_classes, model.num_anchors, name=name, bbox=True, base=model, anchor_params=anchor_params,
                 nms=apply_nms, class_specific_filter=class_specific_filter)


def resnet_retinanet(num_classes, backbone='resnet50', inputs=None, modifier=None, **kwargs):
    """ model/defineModel.py:357-389."""
    if backbone not in ('resnet50', 'resnet101', 'resnet152'):
        raise ValueError('Backbone (\'{}\') is invalid.'.format(backbone))
    m = retinanet(inputs=inputs, num_classes=num_classes, backbone_layers=None, backbone=backbone, **kwargs)
    if modifier:                                  # on the ResNet only, as the reference (:384-386): the FPN and the heads still train
        modifier(m.backbone_view())
    return m


def resnet50_retinanet(num_classes, inputs=None, **kwargs):
    return resnet_retinanet(num_classes=num_classes, backbone='resnet50', inputs=inputs, **kwargs)


def resnet101_retinanet(num_classes, inputs=None, **kwargs):
    return resnet_retinanet(num_classes=num_classes, backbone='resnet101', inputs=inputs, **kwargs)


def resnet152_retinanet(num_classes, inputs=None, **kwargs):
    return resnet_retinanet(num_classes=num_classes, backbone='resnet152', inputs=inputs, **kwargs)
