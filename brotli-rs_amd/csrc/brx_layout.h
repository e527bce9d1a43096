// brx_layout.h -- where the areas of a decoder wave's LDS lie, for every instance of the kernel.  THE place these numbers live:
// brx_device.h (host and kernels), struct Lds of brx_kernels.hip (checked field by field against this file), the two assembly
// loops (brx_hot.S, brx_lens.S) and tools/asm_emu.py all read them from here.
//
// Preprocessor arithmetic on plain integers only -- no suffixes, casts or declarations -- so that hipcc and
// `cpp -x assembler-with-cpp` both take it.  Selected by BRX_LEVEL (0 .. 4, default 0) and BRX_SMALL (the lean instance); the
// table of the instances is in brx_device.h.
#ifndef BRX_LAYOUT_H
#define BRX_LAYOUT_H

#ifndef BRX_LEVEL
#define BRX_LEVEL 0
#endif
#define BRX_L_PASTE_(a, b) a##b
#define BRX_L_PASTE(a, b) BRX_L_PASTE_(a, b) // (b expanded first: BRX_L_PASTE(x_, BRX_LEVEL) = x_0 .. x_4)

// A wider level has that many more bytes of table memory than level 0, and nothing else.
#define BRX_L_GROW_0 0
#define BRX_L_GROW_1 2560
#define BRX_L_GROW_2 10240
#define BRX_L_GROW_3 30720
#define BRX_L_GROW_4 143360
#define BRX_L_GROW_OF(k) ((k) == 0 ? BRX_L_GROW_0 : (k) == 1 ? BRX_L_GROW_1 : (k) == 2 ? BRX_L_GROW_2 : (k) == 3 ? BRX_L_GROW_3 : BRX_L_GROW_4)
#define BRX_L_TM_WORDS_AT(grow) (1728 + (grow) / 4)
#define BRX_L_BYTES_AT(grow) (10240 + (grow))
#define BRX_L_TM_WORDS_OF(k) BRX_L_TM_WORDS_AT(BRX_L_GROW_OF(k)) // table-memory words of level k
#define BRX_L_BYTES_OF(k) BRX_L_BYTES_AT(BRX_L_GROW_OF(k))       // LDS bytes of level k
#define BRX_L_ST_LEVEL0 9728 // byte offset of Lds::st at level 0, whatever the selected instance (BrxResume::lds parks that layout)

// Sizes that no instance changes.  During the command loop brx_hot.S keeps three tables of 256 B in `lens`: ITAB, SPARE, CMH.
#define BRX_L_RING 0
#define BRX_L_RING_BYTES 2048
#define BRX_L_LENS_BYTES 768
#define BRX_L_ST_BYTES 192
#define BRX_L_MBW_BYTES 192
#define BRX_L_TRASH_BYTES 64

// Byte offsets of the selected instance.  The assembly loops paste these behind `offset:`, and the generated text is compared
// from build to build: the offsets are written the way they are to appear there, and verified below.
#if defined(BRX_SMALL)
// the lean instance: ring, 512 words of tables, lens, trash, pad -- no st / mbw, no assembly loop but brx_lens.S
#define BRX_L_TM_WORDS 512
#define BRX_L_TM 2048
#define BRX_L_LENS 4096
#define BRX_L_TRASH 4864
#define BRX_L_PAD 4928
#define BRX_L_PAD_BYTES 192
#define BRX_L_BYTES 5120
#else
#define BRX_L_GROW BRX_L_PASTE(BRX_L_GROW_, BRX_LEVEL)
#define BRX_L_TM_WORDS BRX_L_TM_WORDS_AT(BRX_L_GROW)
#define BRX_L_BYTES BRX_L_BYTES_AT(BRX_L_GROW)
#define BRX_L_PAD_BYTES 64
#if BRX_LEVEL == 4
// level 4: the table memory LAST -- every other area keeps an offset a DS instruction's 16-bit immediate can hold
#define BRX_L_LENS 2048
#define BRX_L_ITAB 2048
#define BRX_L_SPARE 2304
#define BRX_L_CMH 2560
#define BRX_L_ST 2816
#define BRX_L_MBW 3008
#define BRX_L_PAD 3200
#define BRX_L_TRASH 3264
#define BRX_L_TM 3328
#else
// levels 0 .. 3: ring, table memory, then everything else -- that much further up, the wider the level
#define BRX_L_TM 2048
#if BRX_LEVEL == 0
#define BRX_L_LENS 8960
#elif BRX_LEVEL == 1
#define BRX_L_LENS 11520
#elif BRX_LEVEL == 2
#define BRX_L_LENS 19200
#elif BRX_LEVEL == 3
#define BRX_L_LENS 39680
#endif
#define BRX_L_ITAB (8960+BRX_L_GROW)   // byte -> context info (filled by prepare_fast_tables)
#define BRX_L_SPARE (9216+BRX_L_GROW)  // 12 x 4 B: the two-entry symbol lists of resident one-symbol literal trees
#define BRX_L_CMH (9472+BRX_L_GROW)    // context id * 4 -> tree descriptor of the current literal block type (filled at entry)
#define BRX_L_ST (9728+BRX_L_GROW)
#define BRX_L_MBW (9920+BRX_L_GROW)
#define BRX_L_PAD (10112+BRX_L_GROW)
#define BRX_L_TRASH (10176+BRX_L_GROW)
#endif
#endif

// ---- the numbers above agree with each other (struct Lds is checked against them in brx_kernels.hip)
#if BRX_L_ST_LEVEL0 != BRX_L_RING_BYTES + 4 * BRX_L_TM_WORDS_OF(0) + BRX_L_LENS_BYTES
#error "brx_layout.h: BRX_L_ST_LEVEL0 is not where level 0's ring, table memory and lens end"
#endif
#if defined(BRX_SMALL)
#if BRX_L_TM != BRX_L_RING_BYTES || BRX_L_LENS != BRX_L_TM + 4 * BRX_L_TM_WORDS || BRX_L_TRASH != BRX_L_LENS + BRX_L_LENS_BYTES || \
    BRX_L_PAD != BRX_L_TRASH + BRX_L_TRASH_BYTES || BRX_L_BYTES != BRX_L_PAD + BRX_L_PAD_BYTES
#error "brx_layout.h: the lean instance's offsets do not follow from its sizes"
#endif
#else
#if BRX_LEVEL < 0 || BRX_LEVEL > 4
#error "brx_layout.h: BRX_LEVEL is 0 .. 4"
#endif
#if BRX_L_ITAB != BRX_L_LENS || BRX_L_SPARE != BRX_L_ITAB + 256 || BRX_L_CMH != BRX_L_SPARE + 256 || BRX_L_ST != BRX_L_CMH + 256 || \
    BRX_L_ST != BRX_L_LENS + BRX_L_LENS_BYTES || BRX_L_MBW != BRX_L_ST + BRX_L_ST_BYTES || BRX_L_PAD != BRX_L_MBW + BRX_L_MBW_BYTES || \
    BRX_L_TRASH != BRX_L_PAD + BRX_L_PAD_BYTES
#error "brx_layout.h: the offsets behind `lens` do not follow from the sizes"
#endif
#if BRX_LEVEL == 4
#if BRX_L_LENS != BRX_L_RING_BYTES || BRX_L_TM != BRX_L_TRASH + BRX_L_TRASH_BYTES || BRX_L_BYTES != BRX_L_TM + 4 * BRX_L_TM_WORDS || BRX_L_TM > 65535
#error "brx_layout.h: level 4's offsets do not follow from the sizes"
#endif
#else
#if BRX_L_TM != BRX_L_RING_BYTES || BRX_L_LENS != BRX_L_TM + 4 * BRX_L_TM_WORDS || BRX_L_BYTES != BRX_L_TRASH + BRX_L_TRASH_BYTES
#error "brx_layout.h: the offsets of levels 0 .. 3 do not follow from the sizes"
#endif
#endif
#endif

#endif // BRX_LAYOUT_H
