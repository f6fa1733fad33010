"""Host half of the density text writer (csrc/fmt_core.h, csrc/k_format.h): the values the device leaves to the host,
formatted the way the reference's writers do (utils.py:40-94), and the streamed text of one density block.

The device formats every value it can prove; the rest (nan, inf, subnormals, magnitudes outside the exact integer
range, and for the Fortran style values whose floor(log10) is not certain) come back here:
  E / E_space  Python's own format(v, '.{p}E') / format(v, ' .{p}E') with a leading ' '
  F            numpy's float64 steps of fortran_format applied to those values alone (every step is element-wise,
               so a value's text does not depend on its neighbours)
"""
import numpy as np

STYLES = {'E': 0, 'E_space': 1, 'F': 2}
LAYOUTS = {'chgcar': 0, 'cube': 1}           # Fortran order, 5 per line / C order, records of nz in lines of 6
POW10_LO, POW10_N = -300, 601                # the table np.power(10.0, k) the Fortran style divides by


def style_of(fortran_format):
    """file_info['fortran_format'] -> style name (io/vasp.py write, io/cube.py write)"""
    return {2: 'F', 1: 'E_space'}.get(int(fortran_format or 0), 'E')


def pow10_table():
    """np.power(10.0, k) for POW10_LO <= k < POW10_LO + POW10_N, from the numpy this process runs: numpy's pow is not
    correctly rounded and differs between builds (SVML or not, numpy 1.x / 2.x), and the Fortran style's digits depend
    on it exactly as the reference's do"""
    return np.power(10.0, np.arange(POW10_LO, POW10_LO + POW10_N, dtype=np.int64))


def host_strings(vals, style, prec, p10=None):
    """the text of each value in `vals` (already scaled), as the reference's formatter writes it (F: the powers of ten
    from `p10`, the table handed to the device, where it has them)"""
    vals = np.asarray(vals, dtype=np.float64).ravel()
    if style in ('E', 'E_space'):
        spec = ('%s.%dE' % (' ' if style == 'E_space' else '', prec))
        return [' ' + format(float(v), spec) for v in vals]
    if style != 'F':
        raise ValueError(f'unknown style {style!r}')
    a = vals.reshape(-1, 1)
    mag = np.abs(a)
    nz = np.where(a != 0)
    ex = np.zeros(a.shape, dtype=np.int64)
    value = np.zeros(a.shape, dtype=np.int64)
    with np.errstate(all='ignore'):
        ex[nz] = np.floor(np.log10(mag[nz])) + 1
        abs_ex = np.abs(ex)
        k = ex[nz] - prec
        p = np.power(10.0, k)
        p10 = pow10_table() if p10 is None else p10
        inside = (k >= POW10_LO) & (k < POW10_LO + POW10_N)
        p[inside] = p10[k[inside] - POW10_LO]
        value[nz] = 0.5 + mag[nz] / p
    digits = np.full(a.shape, '0' * prec, dtype=f'<U{prec}')
    digits[nz] = value[nz]
    e2 = np.full(a.shape, '0', dtype='<U2')
    e2[nz] = abs_ex[nz]
    out = []
    for i in range(a.shape[0]):
        sign = ' -.' if a[i, 0] < 0 else ' 0.'
        out.append(sign + str(digits[i, 0]) + ('E-' if ex[i, 0] < 0 else 'E+') + ('0' if abs_ex[i, 0] < 10 else '')
                   + str(e2[i, 0]))
    return out


def write_block(f, ctx, values, scale, style, prec, layout):
    """format `values` ([x][y][z] float64, times `scale`) on the device and write the text to the open binary file
    `f` chunk by chunk; returns the number of values the host formatted"""
    n_host = 0
    for chunk, n in ctx.format_density_text(values, scale, style, prec, layout):
        f.write(chunk)
        n_host = n
    return n_host
