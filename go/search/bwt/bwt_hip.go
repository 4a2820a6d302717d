// Drop-in addition to github.com/bebop/poly/search/bwt over libpolyhip.
//
// The reference's bwt.go stays as it is (no declaration is renamed: New, Count, Locate, Extract, Len and GetTransform keep
// the reference's bodies).  This file adds a device-resident index beside it: NewIndex builds the suffix array, the last
// column and the occurrence structure on the GPU, and Count / Locate / Extract / Len / GetTransform answer as the reference
// does, plus CountBatch and LocateBatch for batches of patterns.  UNCOMPILED here (no Go toolchain in the authoring image).
package bwt

import (
	"errors"
	"fmt"

	"github.com/bebop/poly/internal/polyhip"
)

// Index is the GPU FM-index of one sequence; Close releases its device memory.
type Index struct {
	dev *polyhip.BWT
	n   int
}

// NewIndex: the reference's New (bwt.go:455-517) on the device, with the same errors.
func NewIndex(sequence string) (*Index, error) {
	if err := validateSequenceBeforeTransforming(&sequence); err != nil {
		return nil, err
	}
	d, err := polyhip.NewBWT([]byte(sequence))
	if err != nil {
		return nil, err
	}
	return &Index{dev: d, n: len(sequence)}, nil
}

func (ix *Index) Close() { ix.dev.Close() }

// Len (bwt.go:301-304).
func (ix *Index) Len() int { return ix.n }

// GetTransform (bwt.go:306-323).
func (ix *Index) GetTransform() string {
	l, err := ix.dev.Transform()
	if err != nil {
		panic(err)
	}
	return string(l)
}

// CountBatch: Count (bwt.go:235-247) of every pattern; an empty pattern fails the batch with the reference's error.
func (ix *Index) CountBatch(patterns []string) ([]int, error) {
	buf, offs := polyhip.Pack(patterns)
	start, end, errs, err := ix.dev.CountBatch(buf, offs)
	if err != nil {
		return nil, err
	}
	counts := make([]int, len(patterns))
	for i := range counts {
		if errs[i] != 0 {
			return nil, errors.New("Pattern can not be empty")
		}
		counts[i] = int(end[i]) - int(start[i])
	}
	return counts, nil
}

// LocateBatch: Locate (bwt.go:249-273) of every pattern, in suffix-array row order; nil where nothing matches.
func (ix *Index) LocateBatch(patterns []string) ([][]int, error) {
	buf, offs := polyhip.Pack(patterns)
	first, out, errs, err := ix.dev.LocateBatch(buf, offs, 4*len(patterns))
	if err != nil {
		return nil, err
	}
	res := make([][]int, len(patterns))
	for i := range res {
		if errs[i] != 0 {
			return nil, errors.New("Pattern can not be empty")
		}
		if first[i+1] == first[i] {
			continue
		}
		res[i] = make([]int, first[i+1]-first[i])
		for j := range res[i] {
			res[i][j] = int(out[first[i]+uint64(j)])
		}
	}
	return res, nil
}

func (ix *Index) Count(pattern string) (int, error) {
	c, err := ix.CountBatch([]string{pattern})
	if err != nil {
		return 0, err
	}
	return c[0], nil
}

func (ix *Index) Locate(pattern string) ([]int, error) {
	r, err := ix.LocateBatch([]string{pattern})
	if err != nil {
		return nil, err
	}
	return r[0], nil
}

// Extract (bwt.go:275-299), the reference's checks in the reference's order.
func (ix *Index) Extract(start, end int) (string, error) {
	if err := validateRange(start, end); err != nil {
		return "", err
	}
	if end > ix.n {
		return "", fmt.Errorf("end [%d] exceeds the max range of the BWT [%d]", end, ix.n)
	}
	if start < 0 {
		return "", fmt.Errorf("start [%d] exceeds the min range of the BWT [0]", start)
	}
	out, errs, err := ix.dev.ExtractBatch([]int64{int64(start)}, []int64{int64(end)}, []uint64{0, uint64(end - start)})
	if err != nil {
		return "", err
	}
	if errs[0] != 0 {
		return "", fmt.Errorf("polyhip: extract error %d", errs[0])
	}
	return string(out), nil
}

// MismatchHit is one position of the sequence at which a pattern occurs with Mismatches substitutions.
type MismatchHit struct{ Pos, Mismatches int }

// CountMismatchBatch: per pattern, the positions at Hamming distance exactly 0..k (k <= 4):
// substitutions only, matches inside the sequence, bytes compared raw.  An empty pattern fails the batch as Count does.
func (ix *Index) CountMismatchBatch(patterns []string, k int) ([][]int, error) {
	buf, offs := polyhip.Pack(patterns)
	counts, errs, err := ix.dev.CountMismatchBatch(buf, offs, k)
	if err != nil {
		return nil, err
	}
	res := make([][]int, len(patterns))
	for i := range res {
		if errs[i] != 0 {
			return nil, errors.New("Pattern can not be empty")
		}
		res[i] = make([]int, k+1)
		for d := range res[i] {
			res[i][d] = int(counts[i*(k+1)+d])
		}
	}
	return res, nil
}

// LocateMismatchBatch: per pattern, every hit with at most k mismatches, ascending by position; nil where there is none.
func (ix *Index) LocateMismatchBatch(patterns []string, k int) ([][]MismatchHit, error) {
	buf, offs := polyhip.Pack(patterns)
	first, pos, mm, errs, err := ix.dev.LocateMismatchBatch(buf, offs, k, 4*len(patterns))
	if err != nil {
		return nil, err
	}
	res := make([][]MismatchHit, len(patterns))
	for i := range res {
		if errs[i] != 0 {
			return nil, errors.New("Pattern can not be empty")
		}
		for j := first[i]; j < first[i+1]; j++ {
			res[i] = append(res[i], MismatchHit{Pos: int(pos[j]), Mismatches: int(mm[j])})
		}
	}
	return res, nil
}

func (ix *Index) CountMismatch(pattern string, k int) ([]int, error) {
	c, err := ix.CountMismatchBatch([]string{pattern}, k)
	if err != nil {
		return nil, err
	}
	return c[0], nil
}

func (ix *Index) LocateMismatch(pattern string, k int) ([]MismatchHit, error) {
	r, err := ix.LocateMismatchBatch([]string{pattern}, k)
	if err != nil {
		return nil, err
	}
	return r[0], nil
}
