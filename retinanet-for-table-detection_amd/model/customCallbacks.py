"""model/customCallbacks.py of the reference (RedirectModel) and the evaluation callback its training script leaves a slot for
(RetinaNet.py:149, "Callback : Evaluation"): Evaluate computes AP / P / R / F1 on a validation generator at the end of every epoch,
on the device (model/eval.py evaluate_generator), and writes them into the epoch's logs, so callbacks that come after it in the
list (ModelCheckpoint(monitor='mAP')-style) can select by them.  Validate does the same in one pass that also yields the validation
loss (model/eval.py validate_generator): `val_loss` - what the reference's ModelCheckpoint monitors, RetinaNet.py:153-161 - and mAP
from one forward per group.  Model.fit_generator calls set_model / on_train_begin / on_epoch_begin / on_epoch_end / on_train_end in
list order; the Keras callbacks of RetinaNet.py's create_callbacks are in model/callbacks.py."""
from . import eval as _eval


class RedirectModel:
    """Callback which wraps another callback, but executed on a different model (reference model/customCallbacks.py):
    RedirectModel(Evaluate(generator), prediction_model) evaluates prediction_model while the training model trains."""

    def __init__(self, callback, model):
        self.callback = callback
        self.redirect_model = model

    def set_model(self, model):
        # fit_generator hands every callback the training model: the wrapped one gets the redirect model instead
        self.model = model
        if hasattr(self.callback, "set_model"):
            self.callback.set_model(self.redirect_model)

    def _forward(self, name, *args, **kwargs):
        fn = getattr(self.callback, name, None)
        if fn is not None:
            fn(*args, **kwargs)

    def on_epoch_begin(self, epoch, logs=None):
        self._forward("on_epoch_begin", epoch, logs=logs)

    def on_epoch_end(self, epoch, logs=None):
        self._forward("on_epoch_end", epoch, logs=logs)

    def on_batch_begin(self, batch, logs=None):
        self._forward("on_batch_begin", batch, logs=logs)

    def on_batch_end(self, batch, logs=None):
        self._forward("on_batch_end", batch, logs=logs)

    def on_train_begin(self, logs=None):
        if hasattr(self.callback, "set_model"):
            self.callback.set_model(self.redirect_model)
        self._forward("on_train_begin", logs=logs)

    def on_train_end(self, logs=None):
        self._forward("on_train_end", logs=logs)


class Evaluate:
    """Evaluation of a generator's pages at the end of every epoch.

    logs['mAP']: mean over the IoU thresholds of the mean AP over the classes with annotations (weighted_average=True: weighted by
    their annotation counts); with a single threshold that is mAP at that threshold.  logs['weighted_f1'] (when more than one
    threshold is given): sum_t t * F1_t / sum_t t at f1_score_threshold.  The model evaluated is the callback's model if it is an
    inference model, else the inference model on top of it (retinanet_bbox(model=...)), which shares its engine and therefore the
    weights as trained so far.  `evaluate` replaces model/eval.py's evaluate_generator (same signature), e.g. in tests."""

    def __init__(self, generator, iou_thresholds=(0.5,), score_threshold=0.05, max_detections=300, f1_score_threshold=0.5,
                 weighted_average=False, in_flight=2, verbose=1, evaluate=None):
        self.generator = generator
        self.iou_thresholds = tuple(float(t) for t in iou_thresholds)
        self.score_threshold, self.max_detections, self.f1_score_threshold = score_threshold, max_detections, f1_score_threshold
        self.weighted_average, self.in_flight, self.verbose = bool(weighted_average), in_flight, verbose
        self.evaluate = evaluate or _eval.evaluate_generator
        self.model = None
        self.result = None

    def set_model(self, model):
        self.model = model

    def _inference_model(self):
        if getattr(self.model, "bbox", False):
            return self.model
        from .defineModel import retinanet_bbox
        return retinanet_bbox(model=self.model)

    def on_epoch_end(self, epoch, logs=None):
        logs = logs if logs is not None else {}
        r = self.evaluate(self._inference_model(), self.generator, iou_thresholds=self.iou_thresholds,
                          score_threshold=self.score_threshold, max_detections=self.max_detections,
                          f1_score_threshold=self.f1_score_threshold, in_flight=self.in_flight)
        self.result = r
        if self.weighted_average:
            per_t = [_eval.mean_ap(r["average_precision"][t], weighted=True) for t in r["iou_thresholds"]]
            logs['mAP'] = float(sum(per_t) / len(per_t))
        else:
            logs['mAP'] = float(r["mAP"])
        if len(self.iou_thresholds) > 1:
            logs['weighted_f1'] = float(r["weighted_f1"])
        if self.verbose:
            line = "mAP: %.4f" % logs['mAP']
            if 'weighted_f1' in logs:
                line += " - weighted_f1: %.4f" % logs['weighted_f1']
            print("Epoch %d evaluation - %s" % (epoch + 1, line))
        return logs


class Validate(Evaluate):
    """Evaluate plus the validation loss, from ONE pass over the generator at the end of every epoch (validate_generator): besides
    logs['mAP'] (and logs['weighted_f1'] with more than one threshold) it writes logs['val_loss'], logs['val_regression_loss'] and
    logs['val_classification_loss'] - Keras' evaluate_generator numbers on the generator's pages without augmentation - so
    ModelCheckpoint(monitor='val_loss'), EarlyStopping and ReduceLROnPlateau placed after it in the list select by them.
    Takes Evaluate's arguments and is wrapped by RedirectModel the same way; alpha / gamma / sigma are the losses' parameters
    (model/losses.py).  `result['image_losses']` lists each page's share of the loss."""

    def __init__(self, generator, iou_thresholds=(0.5,), score_threshold=0.05, max_detections=300, f1_score_threshold=0.5,
                 weighted_average=False, in_flight=2, verbose=1, evaluate=None, alpha=0.25, gamma=2.0, sigma=3.0):
        super(Validate, self).__init__(generator, iou_thresholds, score_threshold, max_detections, f1_score_threshold,
                                       weighted_average, in_flight, verbose, evaluate or self._validate)
        self.alpha, self.gamma, self.sigma = alpha, gamma, sigma

    def _validate(self, model, generator, **kw):
        return _eval.validate_generator(model, generator, alpha=self.alpha, gamma=self.gamma, sigma=self.sigma, **kw)

    def on_epoch_end(self, epoch, logs=None):
        logs = logs if logs is not None else {}
        verbose, self.verbose = self.verbose, 0
        try:
            super(Validate, self).on_epoch_end(epoch, logs)
        finally:
            self.verbose = verbose
        r = self.result
        logs['val_loss'] = float(r["loss"])
        logs['val_regression_loss'] = float(r["regression_loss"])
        logs['val_classification_loss'] = float(r["classification_loss"])
        if self.verbose:
            line = "val_loss: %.4f - mAP: %.4f" % (logs['val_loss'], logs['mAP'])
            if 'weighted_f1' in logs:
                line += " - weighted_f1: %.4f" % logs['weighted_f1']
            print("Epoch %d validation - %s" % (epoch + 1, line))
        return logs
