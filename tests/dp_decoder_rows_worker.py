"""One rank of the two-rank data-parallel check with model.decoder_rows (launched by tests/test_gpu_decoder_rows_dp.py): the rank
of tests/dp_worker.py, unchanged, on a model whose enhanced mask decoder runs on the labelled rows only."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import tests.dp_worker as W
    import tests.test_gpu_model as M

    build = M.build

    def build_on(*a, **k):
        m = build(*a, **k)
        m.decoder_rows = True
        return m

    M.build = build_on  # dp_worker.main() imports `build` from there when it runs
    W.main()


if __name__ == "__main__":
    main()
