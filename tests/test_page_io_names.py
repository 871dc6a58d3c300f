"""model/page_io.py is the one home of the page-file functions; csv_generator.py and model/utils.py, where the reference's layout
has them, re-export the public names.  Needs no GPU: only names are looked at."""
import importlib
import os
import subprocess
import sys

PKG = "retinanet-for-table-detection_amd"
PKG_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), PKG)
FROM_CSV_GENERATOR = ("read_image_bgr", "read_images_bgr", "jpeg_inspect", "png_inspect", "_decode_batch")
FROM_UTILS = ("write_image", "write_images_bgr", "encode_jpeg_bgr", "encode_png_bgr", "decode_png_bgr", "JPEG_EXTENSIONS")
NOT_REEXPORTED = ("_decode_datas", "_readers", "_readers_lock", "_reader", "_check_page", "_check_settings", "_host_page", "_pillow_jpeg",
                  "_files_to_host", "_encode_batch")


def test_old_names_are_the_page_io_objects():
    pio = importlib.import_module(PKG + ".model.page_io")
    for old, names in (("csv_generator", FROM_CSV_GENERATOR), ("model.utils", FROM_UTILS),
                       ("model.preprocess", ("read_images_bgr", "write_images_bgr"))):
        mod = importlib.import_module(PKG + "." + old)
        for name in names:
            assert getattr(mod, name) is getattr(pio, name), (old, name)
        for name in NOT_REEXPORTED:
            assert hasattr(pio, name) and not hasattr(mod, name), (old, name)


def test_csv_generator_loads_top_level():
    """The reference's layout: the package directory first on sys.path, `import csv_generator`, in a fresh interpreter."""
    code = ("import sys; sys.path.insert(0, %r); import csv_generator, model.page_io as pio; "
            "assert callable(csv_generator.read_images_bgr) and csv_generator.read_images_bgr is pio.read_images_bgr; "
            "assert csv_generator.__name__ == 'csv_generator' and pio.__name__ == 'model.page_io'; print('top-level ok')" % PKG_DIR)
    out = subprocess.check_output([sys.executable, "-c", code], text=True)
    assert out.strip().splitlines()[-1] == "top-level ok"
