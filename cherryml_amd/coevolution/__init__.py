from ._scan import (CoevolutionScanner, average_product_correction, coevolution_scan,  # noqa: F401
                    read_coevolution_scan)
